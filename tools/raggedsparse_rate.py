"""Problem-iterations per second of the ragged sparse batch (totsu_amd.RaggedSparseBatchSolver: sparse problems of different shapes,
cone layouts and patterns in one batch) against the two earlier routes for such a set, in one process on one device, eps_acc = 1e-30
so that nothing stops:

  route 1 (bucketed)   bucket the problems by identical (n, m, cone layout) and run one SparseBatchSolver per bucket, one after the other;
  route 2 (densified)  one RaggedBatchSolver on the dense matrices.

Seeded workloads at P = 256 and P = 1024 problems:

  (p)  partitioning_sdp on a spread of grids from (2, 2) to (4, 8): one PSD cone of order rows x columns and as many equality rows,
       one entry per row of A -- the graph relaxations on graphs of different size;
  (l1), (l5)  sparse LPs over the nonnegative cone with every shape unique, n spread over 32 .. 512, m = 2 n (+ r), at 1 % and at 5 %
       density -- so every bucket of route 1 holds one problem;
  (u)  a uniform partitioning_sdp(4, 8) set: the ragged sparse batch against SparseBatchSolver itself on the same problems, which
       prices the descriptor, the per-problem residency flag and the forced live list.

Every route is timed twice, alternating, so that the spread of a route against itself stands beside the difference between routes.
Host clock around run() with the stream synchronised; construction, init and a warm-up run are outside the timed span.  A timed
window lasts about --window seconds and is taken three times: the median is reported, with the spread.  The info() of each batch is
written beside the rates.  No ratio is a condition: the figures are what they are.  profiles/raggedsparse_rate.txt.
    python tools/raggedsparse_rate.py [--window 0.3] [--poll 32] [--sizes 256,1024] [--mixes p,l1,l5,u] [--out profiles/raggedsparse_rate.txt]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from midbatch_rate import F, T, _lib, compute_units  # noqa: E402  (puts the package and tests/ on the path)
from raggedbatch_rate import Dense, of_family, rate_of  # noqa: E402
from sdpbatch_rate import partitioning_family  # noqa: E402

GRIDS = [(2, 2), (2, 3), (2, 4), (3, 3), (2, 5), (3, 4), (2, 7), (3, 5), (4, 4), (3, 6), (4, 5), (3, 7), (4, 6), (3, 8), (4, 7), (4, 8)]


def sparse_lp(m, n, density, seed):
    """a primal- and dual-feasible sparse LP over the nonnegative cone: b = A x0 + s0, c = -A^T y0, s0, y0 ~ U(0.1, 1.1)"""
    rng = np.random.default_rng(1000 * m + n + 7919 * seed + int(1e4 * density))
    A = (rng.standard_normal((n, m), dtype=F) / F(np.sqrt(max(density * n, 1.0)))) * (rng.random((n, m), dtype=F) < density)
    A = A.astype(F)                                                        # (n, m) row-major is (m, n) column-major
    x0, s0, y0 = rng.standard_normal(n).astype(F), rng.uniform(0.1, 1.1, m).astype(F), rng.uniform(0.1, 1.1, m).astype(F)
    return Dense(n, m, A.ravel(), x0 @ A + s0, -(A @ y0), [_lib.CONE_RPOS], [m])


def mix_lp(P, density):
    ns = [32 + (k * 480) // (P - 1) for k in range(P)]
    seen, out = {}, []
    for k, n in enumerate(ns):
        r = seen.get(n, 0)
        seen[n] = r + 1
        out.append(sparse_lp(2 * n + r, n, density, k))
    assert len({(d.n, d.m) for d in out}) == P
    return out


def buckets(ds):
    out = {}
    for d in ds:
        out.setdefault((d.n, d.m, tuple(d.seg_type), tuple(d.seg_len)), []).append(d)
    return list(out.values())


def short(info):
    keep = ("n_prob", "threads", "lds_bytes", "n_layouts", "n_resident", "resident", "nnz_cap", "nnz_total", "blob_bytes", "arena_bytes",
            "device_bytes", "a_bytes_per_iter", "n_load16", "max_psd_order")
    out = {k: info[k] for k in keep if k in info}
    if "classes" in info:
        out["classes"] = [{k: c[k] for k in ("n_prob", "threads", "lds_bytes", "n_resident") if k in c} for c in info["classes"]]
    return out


def one_rate(make, count, a):
    sb = make()
    out = rate_of(lambda it: sb.run(it, a.poll), count, a, lambda: [sb.status(0), sb.status(count - 1)])
    info = sb.info()
    sb.destroy()
    return out, info


def bucketed_rate(ds, p, a):
    sbs = [T.SparseBatchSolver.from_dense(b, p) for b in buckets(ds)]
    out = rate_of(lambda it: [sb.run(it, a.poll) for sb in sbs], len(ds), a, lambda: [sb.status(0) for sb in (sbs[0], sbs[-1])])
    infos = [sb.info() for sb in sbs]
    for sb in sbs:
        sb.destroy()
    return out, {"buckets": len(sbs), "resident": sum(i["resident"] for i in infos), "blob_bytes": sum(i["blob_bytes"] * i["n_prob"] for i in infos),
                 "device_bytes": sum(i["device_bytes"] for i in infos)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--poll", type=int, default=32)
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--mixes", default="p,l1,l5,u")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    p = T.SolverParam()
    p.eps_acc = 1e-30
    mixes = a.mixes.split(",")
    say("raggedsparse_rate: problem-iterations per second, eps_acc = 1e-30 (nothing stops), poll_every = %d, %d CUs" % (a.poll, compute_units()))
    say("   new: one RaggedSparseBatchSolver over the whole set; bucketed: one SparseBatchSolver per distinct (n, m, layout), in turn;")
    say("   densified: one RaggedBatchSolver on the dense matrices.  Windows of about %.2f s, median of 3 (low .. high), two runs each" % a.window)
    fams = [partitioning_family(g) for g in GRIDS] if "p" in mixes or "u" in mixes else None
    summary = []
    what = {"p": "partitioning_sdp on %d grids from (2, 2) to (4, 8)" % len(GRIDS), "l1": "sparse LPs, every shape unique, n = 32 .. 512, m = 2 n (+ r), 1 %",
            "l5": "sparse LPs, every shape unique, n = 32 .. 512, m = 2 n (+ r), 5 %"}
    for P in [int(v) for v in a.sizes.split(",")]:
        for mix in mixes:
            if mix == "u":
                continue
            ds = [of_family(fams[k % len(fams)], k // len(fams)) for k in range(P)] if mix == "p" else mix_lp(P, 0.01 if mix == "l1" else 0.05)
            say()
            say("(%s) P = %d: %s" % (mix, P, what[mix]))
            got = {"new": [], "bucketed": [], "densified": []}
            for _ in range(2):
                got["new"].append(one_rate(lambda: T.RaggedSparseBatchSolver.from_dense(ds, p), P, a))
                got["bucketed"].append(bucketed_rate(ds, p, a))
                got["densified"].append(one_rate(lambda: T.RaggedBatchSolver.from_dense(ds, p), P, a))
            for k in ("new", "bucketed", "densified"):
                for q, ((r, lo, hi, it), info) in enumerate(got[k]):
                    say("   %-9s run %d  %6d iterations per window  %11.0f problem-iterations/s (%.0f .. %.0f)" % (k, q + 1, it, r, lo, hi))
                say("   %-9s info %s" % (k, short(got[k][0][1]) if k != "bucketed" else got[k][0][1]))
            mean = {k: sum(g[0][0] for g in got[k]) / 2 for k in got}
            say("   new / bucketed %.2f, new / densified %.2f (means of the two runs); run 2 / run 1: new %.3f, bucketed %.3f, densified %.3f"
                % (mean["new"] / mean["bucketed"], mean["new"] / mean["densified"], *(got[k][1][0][0] / got[k][0][0][0] for k in got)))
            summary.append("(%s) P=%d %.2f / %.2f" % (mix, P, mean["new"] / mean["bucketed"], mean["new"] / mean["densified"]))
            flush()
        if "u" in mixes:
            ds = [of_family(fams[-1], k) for k in range(P)]
            say()
            say("(u) P = %d: uniform partitioning_sdp(4, 8), 560 x 528 with 560 entries, the ragged sparse batch against SparseBatchSolver, alternating" % P)
            got = {"new": [], "sparse": []}
            for _ in range(2):
                got["new"].append(one_rate(lambda: T.RaggedSparseBatchSolver.from_dense(ds, p), P, a))
                got["sparse"].append(one_rate(lambda: T.SparseBatchSolver.from_dense(ds, p), P, a))
            for k in ("new", "sparse"):
                for q, ((r, lo, hi, it), info) in enumerate(got[k]):
                    say("   %-7s run %d  %6d iterations per window  %11.0f problem-iterations/s (%.0f .. %.0f)" % (k, q + 1, it, r, lo, hi))
                say("   %-7s info %s" % (k, short(got[k][0][1])))
            nn, ss = [g[0][0] for g in got["new"]], [g[0][0] for g in got["sparse"]]
            say("   new / sparse %.3f (means of the two runs); run 2 / run 1 of the same class: new %.3f, sparse %.3f"
                % (sum(nn) / sum(ss), nn[1] / nn[0], ss[1] / ss[0]))
            summary.append("(u) P=%d %.3f" % (P, sum(nn) / sum(ss)))
            flush()
    say()
    say("ratios (new / bucketed / densified; (u): new / SparseBatchSolver): " + "; ".join(summary))
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
