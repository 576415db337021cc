"""Problem-iterations per second of the sparse own-A batch (totsu_amd.SparseBatchSolver: a problem's entries packed, held in LDS when
they fit, walked by the pass) against the only route such problems had before it -- the same problems DENSIFIED, in SdpBatchSolver
(layouts with PSD cones) or MidBatchSolver -- on

    560 x 528    partitioning_sdp(4, 8): order 32 and 32 zero-cone rows, 560 entries
    512 x 256    LPs, a masked random A at 1 %, 5 %, 25 %, 50 % and 100 % density (where the dense route takes over: the crossover)
    423 x 60     SOCPs (cones of 6, 2, 1, 18, 141, 251, 4 rows), a masked random A at 5 %

at P = 16, 64, 256 and 1024 problems, eps_acc = eps_inf = 1e-30 so that nothing stops, in one process on one device.  Per layout also,
at P = 256: both workgroup sizes, resident against forced-streamed, and the device bytes of A per problem on both routes.  The row
length above which a wave sums a row (SPB_LONG) is a constant of the library: the tool records the one it ran with, and a record of
16 / 32 / 64 is three builds (make -C totsu_amd/csrc CXXEXTRA=-DSPB_LONG=16 after removing thip_sparsebatch.o) and three runs with
--only-sparse.  On the partitioning layout at P = 256 each route is run twice: the margin between the routes is to be read against
the spread of the two runs.

Host clock around run() with the stream synchronised; construction, init and a warm-up run are outside the timed span; a window
lasts about --window seconds, the median of three is reported with the spread (tools/midbatch_rate.py, whose helpers these are).  No
figure is a condition: they are what they are.  profiles/sparsebatch_rate.txt.
    python tools/sparsebatch_rate.py [--window 0.3] [--poll 32] [--sizes 16,64,256,1024] [--only-sparse] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from midbatch_rate import DISTINCT, F, T, _lib, compute_units, stacked, timed  # noqa: E402  (puts the package and tests/ on the path)
from sdpbatch_rate import partitioning_family  # noqa: E402
from totsu_amd import sparsebatch  # noqa: E402

SOC_CONES = [6, 2, 1, 18, 141, 251, 4]


def interior(rng, seg_type, seg_len):
    out = []
    for t, l in zip(seg_type, seg_len):
        if t == _lib.CONE_RPOS:
            v = rng.uniform(0.1, 1.1, l)
        else:
            v = rng.standard_normal(l) / np.sqrt(l)
            v[0] = np.linalg.norm(v[1:]) + rng.uniform(0.5, 1.5)
        out.append(v)
    return np.concatenate(out)


def masked_family(name, m, n, density, seg_type, seg_len):
    """feasible by construction: b = A x0 + s0, c = -A^T y0 with s0, y0 inside the cone"""
    a, b, c = [], [], []
    for s in range(DISTINCT):
        rng = np.random.default_rng(1000 * m + n + 7919 * s + int(1e4 * density))
        A = rng.standard_normal((m, n)) / np.sqrt(max(density * n, 1.0))
        if density < 1.0:
            A *= rng.random((m, n)) < density
        A = A.astype(F).astype(np.float64)
        a.append(np.asfortranarray(A.astype(F)).ravel(order="F"))
        b.append((A @ rng.standard_normal(n) + interior(rng, seg_type, seg_len)).astype(F))
        c.append((-A.T @ interior(rng, seg_type, seg_len)).astype(F))
    return dict(name="%s %d x %d at %g %%" % (name, m, n, 100 * density), n=n, m=m, a=np.stack(a), b=np.stack(b), c=np.stack(c),
                seg_type=list(seg_type), seg_len=list(seg_len))


def windows(sb, P, a):
    sb.run(8, a.poll)                                  # warm-up
    probe = 2 * a.poll
    iters = max(probe, int(probe * a.window / timed(lambda: sb.run(probe, a.poll))) // a.poll * a.poll)
    dts = sorted(timed(lambda: sb.run(iters, a.poll)) for _ in range(3))
    res = [sb.status(i) for i in (0, P - 1)]
    assert all(r.iters == 8 + probe + 3 * iters and r.state == _lib.ST_RUNNING for r in res), [(r.iters, r.state) for r in res]
    return P * iters / dts[1], P * iters / dts[2], P * iters / dts[0]


def dense_rate(cls, fam, P, p, a):
    bufs = [stacked(fam[k], P) for k in ("a", "b", "c")]
    sb = cls(fam["n"], fam["m"], bufs[0], bufs[1], bufs[2], fam["seg_type"], fam["seg_len"], p)
    out = windows(sb, P, a) + (sb.info(),)
    sb.destroy()
    for d in bufs:
        d.free()
    return out


def sparse_rate(fam, mats, P, p, a, **kw):
    bufs = [stacked(fam[k], P) for k in ("b", "c")]
    sb = T.SparseBatchSolver(fam["n"], fam["m"], [mats[i % len(mats)] for i in range(P)], bufs[0], bufs[1], fam["seg_type"],
                             fam["seg_len"], p, **kw)
    out = windows(sb, P, a) + (sb.info(),)
    sb.destroy()
    for d in bufs:
        d.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--poll", type=int, default=32)
    ap.add_argument("--sizes", default="16,64,256,1024")
    ap.add_argument("--only-sparse", action="store_true", help="skip the dense route (a rebuild with another SPB_LONG)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init()
    cus = compute_units()
    long_len = sparsebatch.pack(1, 1, ([0, 0], [], []))[1]
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    p = T.SolverParam()
    p.eps_acc = p.eps_inf = 1e-30
    say("sparsebatch_rate: problem-iterations per second, eps_acc = eps_inf = 1e-30 (nothing stops), poll_every = %d, %d CUs, SPB_LONG = %d"
        % (a.poll, cus, long_len))
    say("   sparse: SparseBatchSolver; dense: the same problems densified in SdpBatchSolver (PSD layouts) or MidBatchSolver")
    say("   windows of about %.2f s, median of 3 (low .. high)" % a.window)
    rpos, soc = _lib.CONE_RPOS, _lib.CONE_SOC
    fams = [lambda: (partitioning_family((4, 8)), T.SdpBatchSolver)]
    fams += [(lambda d=d: (masked_family("LP", 512, 256, d, [rpos], [512]), T.MidBatchSolver)) for d in (0.01, 0.05, 0.25, 0.5, 1.0)]
    fams += [lambda: (masked_family("SOCP", 423, 60, 0.05, [soc] * len(SOC_CONES), SOC_CONES), T.MidBatchSolver)]
    summary = []
    for make in fams:
        fam, dense_cls = make()
        n, m = fam["n"], fam["m"]
        mats = [sparsebatch.csc_of_dense(fam["a"][i], n, m) for i in range(fam["a"].shape[0])]
        nnz = max(int(t[0][-1]) for t in mats)
        lds, thr, res = sparsebatch.fits(n, m, fam["seg_type"], fam["seg_len"], nnz)
        say()
        say("%s  (up to %d entries; A on the device per problem: %d bytes as a blob, %d bytes dense; by rule %d threads, %s)"
            % (fam["name"], nnz, sparsebatch.capacity_bytes(n, m, nnz), 4 * m * n, thr, "resident" if res else "streamed"))
        for P in [int(v) for v in a.sizes.split(",")]:
            sp, slo, shi, info = sparse_rate(fam, mats, P, p, a)
            line = "   P = %-5d sparse %4d threads %6d B LDS %s %10.0f (%.0f .. %.0f)" % (
                P, info["threads"], info["lds_bytes"], "resident" if info["resident"] else "streamed", sp, slo, shi)
            if not a.only_sparse:
                dn, dlo, dhi, dinfo = dense_rate(dense_cls, fam, P, p, a)
                line += "  dense %4d threads %10.0f (%.0f .. %.0f)  sparse / dense %6.2f" % (dinfo["threads"], dn, dlo, dhi, sp / dn)
                summary.append((fam["name"], P, sp / dn))
            say(line)
        P = 256
        for threads in (256, 1024):
            for resident in ((1, 0) if res else (0,)):
                sp, slo, shi, info = sparse_rate(fam, mats, P, p, a, force_threads=threads, force_resident=resident)
                say("   P = %-5d sparse %4d threads forced, %s forced: %10.0f (%.0f .. %.0f); %d bytes of A read per problem-iteration"
                    % (P, threads, "resident" if resident else "streamed", sp, slo, shi, info["a_bytes_per_iter"]))
        if dense_cls is T.SdpBatchSolver and not a.only_sparse:
            runs = {"sparse": [sparse_rate(fam, mats, P, p, a)[0] for _ in range(2)],
                    "dense": [dense_rate(dense_cls, fam, P, p, a)[0] for _ in range(2)]}
            spread = max(abs(v[0] - v[1]) / min(v) for v in runs.values())
            margin = min(runs["sparse"]) / max(runs["dense"]) - 1.0
            say("   P = %-5d two runs of each route: sparse %.0f, %.0f; dense %.0f, %.0f; margin of the sparse route %+.1f %%, "
                "largest spread of two runs %.1f %%" % (P, runs["sparse"][0], runs["sparse"][1], runs["dense"][0], runs["dense"][1],
                                                         100 * margin, 100 * spread))
    if summary:
        say()
        say("sparse / dense: " + "; ".join("%s P=%d %.2f" % s for s in summary))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
