"""Problem-iterations per second of the ragged batch (totsu_amd.RaggedBatchSolver: problems of different shapes and cone layouts in one
batch, one workgroup per running problem, one launch per workgroup-size class and poll) against the only earlier route for such a
set: bucket the problems by identical (n, m, cone layout) and run one conic_batch per bucket, one bucket after the other -- in the
same process on the same device, eps_acc = 1e-30 so that nothing stops.  Three seeded mixes at P = 256 and P = 1024 problems:

  (a) every shape unique: feasible LPs over the nonnegative cone with n spread evenly over 32 .. 512 and m = 2 n + r, r = 0, 1, 2, ..
      counting the earlier problems of the same n (r = 0 throughout at P = 256) -- so every bucket holds one problem;
  (b) four shapes x P / 4: LP 80 x 40, LP 256 x 128, SOCP 423 x 60 (row sums), SDP 45 x 6 of order 9 -- four buckets, which
      conic_batch sends to the small, the mid, the mid and the SDP batch;
  (c) a uniform LP 256 x 128 set: the ragged batch against MidBatchSolver itself on the same problems, which prices the
      descriptor loads and the forced live list.  Both are timed twice, alternating, so that the spread of one class against itself
      stands beside the difference.

Host clock around run() with the stream synchronised; construction, init and a warm-up run are outside the timed span on both
sides.  A timed window lasts about --window seconds (the iteration count is scaled from a first short window; a route whose first
window is already longer keeps that count) and is taken three times: the median is reported, with the spread.  No ratio is a
condition: the figures are what they are.  profiles/raggedbatch_rate.txt.
    python tools/raggedbatch_rate.py [--window 0.3] [--poll 32] [--sizes 256,1024] [--mixes a,b,c] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from midbatch_rate import F, T, _lib, compute_units, lp_family, socp_family, timed  # noqa: E402  (puts the package and tests/ on the path)
from sdpbatch_rate import sdp_family  # noqa: E402

DISTINCT = 16            # problems generated per shape of (b) and (c); larger counts repeat them (every slot streams its own copy)


class Dense:
    """the fields of Prob*.dense()"""

    def __init__(self, n, m, a, b, c, seg_type, seg_len, rowabs=None):
        self.n, self.m, self.mat_a, self.vec_b, self.vec_c = int(n), int(m), a, b, c
        self.seg_type, self.seg_len, self.vec_b_rowabs = list(seg_type), list(seg_len), rowabs


def of_family(fam, i):
    k = i % fam["a"].shape[0]
    ra = fam.get("rowabs")
    return Dense(fam["n"], fam["m"], fam["a"][k], fam["b"][k], fam["c"][k], fam["seg_type"], fam["seg_len"], None if ra is None else ra[k])


def rand_lp(m, n, seed):
    """a primal- and dual-feasible LP over the nonnegative cone: b = A x0 + s0, c = -A^T y0, s0, y0 ~ U(0.1, 1.1)"""
    rng = np.random.default_rng(1000 * m + n + 7919 * seed)
    A = (rng.standard_normal((n, m), dtype=F) / F(np.sqrt(n)))             # (n, m) row-major is (m, n) column-major
    x0, s0, y0 = rng.standard_normal(n).astype(F), rng.uniform(0.1, 1.1, m).astype(F), rng.uniform(0.1, 1.1, m).astype(F)
    return Dense(n, m, A.ravel(), x0 @ A + s0, -(A @ y0), [_lib.CONE_RPOS], [m])


def mix_a(P):
    ns = [32 + (k * 480) // (P - 1) for k in range(P)]
    seen, out = {}, []
    for k, n in enumerate(ns):
        r = seen.get(n, 0)
        seen[n] = r + 1
        out.append(rand_lp(2 * n + r, n, k))
    assert len({(d.n, d.m) for d in out}) == P
    return out


def mix_b(P, fams):
    return [of_family(fams[k % 4], k // 4) for k in range(P)]


def buckets(ds):
    out = {}
    for d in ds:
        out.setdefault((d.n, d.m, tuple(d.seg_type), tuple(d.seg_len), d.vec_b_rowabs is None), []).append(d)
    return list(out.values())


def rate_of(run, count, a, status):
    """(problem-iterations per second: median, low, high; iterations per window) of run(iters), which advances `count` problems"""
    run(8)                                             # warm-up
    probe = 2 * a.poll
    iters = max(probe, int(probe * a.window / timed(lambda: run(probe))) // a.poll * a.poll)
    dts = sorted(timed(lambda: run(iters)) for _ in range(3))
    assert all(r.iters == 8 + probe + 3 * iters and r.state == _lib.ST_RUNNING for r in status()), "a problem stopped"
    return count * iters / dts[1], count * iters / dts[2], count * iters / dts[0], iters


def ragged_rate(ds, p, a):
    rb = T.RaggedBatchSolver.from_dense(ds, p)
    out = rate_of(lambda it: rb.run(it, a.poll), len(ds), a, lambda: [rb.status(0), rb.status(len(ds) - 1)])
    info = rb.info()
    rb.destroy()
    return out, info


def bucketed_rate(ds, p, a):
    sbs = [T.conic_batch(b, p) for b in buckets(ds)]
    out = rate_of(lambda it: [sb.run(it, a.poll) for sb in sbs], len(ds), a, lambda: [sb.status(0) for sb in (sbs[0], sbs[-1])])
    kinds = {}
    for sb in sbs:
        kinds[type(sb).__name__] = kinds.get(type(sb).__name__, 0) + 1
        sb.destroy()
    return out, len(sbs), kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--poll", type=int, default=32)
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--mixes", default="a,b,c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    p = T.SolverParam()
    p.eps_acc = 1e-30
    mixes = a.mixes.split(",")
    say("raggedbatch_rate: problem-iterations per second, eps_acc = 1e-30 (nothing stops), poll_every = %d, %d CUs" % (a.poll, compute_units()))
    say("   ragged: one RaggedBatchSolver over the whole set; bucketed: one conic_batch per distinct (n, m, layout), in turn;")
    say("   windows of about %.2f s, median of 3 (low .. high)" % a.window)
    fams = None
    if "b" in mixes or "c" in mixes:
        fams = [lp_family(40, DISTINCT), lp_family(128, DISTINCT), socp_family(DISTINCT), sdp_family(6, 9)]
    summary = []
    for P in [int(v) for v in a.sizes.split(",")]:
        for mix in mixes:
            if mix == "c":
                continue
            ds = mix_a(P) if mix == "a" else mix_b(P, fams)
            (r, rlo, rhi, rit), info = ragged_rate(ds, p, a)
            (b, blo, bhi, bit), nb, kinds = bucketed_rate(ds, p, a)
            say()
            say("(%s) P = %d: %s" % (mix, P, "every shape unique, LP n = 32 .. 512, m = 2 n (+ r)" if mix == "a" else
                                    "four shapes x %d: LP 80 x 40, LP 256 x 128, SOCP 423 x 60, SDP 45 x 6 order 9" % (P // 4)))
            say("   ragged    classes %s problems at %s B LDS, %d layouts, %d of %d on 16-byte loads, %.1f MB of A per iteration of all"
                % ([c["n_prob"] for c in info["classes"]], [c["lds_bytes"] for c in info["classes"]], info["n_layouts"], info["n_load16"], P,
                   info["a_bytes_per_iter"] / 1e6))
            say("             %6d iterations per window  %11.0f problem-iterations/s (%.0f .. %.0f)" % (rit, r, rlo, rhi))
            say("   bucketed  %d buckets (%s)" % (nb, ", ".join("%d %s" % (v, k) for k, v in sorted(kinds.items()))))
            say("             %6d iterations per window  %11.0f problem-iterations/s (%.0f .. %.0f)" % (bit, b, blo, bhi))
            say("   ratio ragged / bucketed %.2f" % (r / b))
            summary.append("(%s) P=%d %.2f" % (mix, P, r / b))
        if "c" in mixes:
            ds = [of_family(fams[1], k) for k in range(P)]
            say()
            say("(c) P = %d: uniform LP 256 x 128, the ragged batch against MidBatchSolver, alternating" % P)
            got = {"ragged": [], "mid": []}
            for _ in range(2):
                got["ragged"].append(ragged_rate(ds, p, a)[0])
                sb = T.MidBatchSolver.from_dense(ds, p)
                got["mid"].append(rate_of(lambda it: sb.run(it, a.poll), P, a, lambda: [sb.status(0), sb.status(P - 1)]))
                sb.destroy()
            for k in ("ragged", "mid"):
                for q, (r, lo, hi, it) in enumerate(got[k]):
                    say("   %-7s run %d  %6d iterations per window  %11.0f problem-iterations/s (%.0f .. %.0f)" % (k, q + 1, it, r, lo, hi))
            rr, mm = [g[0] for g in got["ragged"]], [g[0] for g in got["mid"]]
            say("   ragged / mid %.3f (means of the two runs); run 2 / run 1 of the same class: ragged %.3f, mid %.3f"
                % (sum(rr) / sum(mm), rr[1] / rr[0], mm[1] / mm[0]))
            summary.append("(c) P=%d %.3f" % (P, sum(rr) / sum(mm)))
    say()
    say("ratios (ragged / the other route): " + "; ".join(summary))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
