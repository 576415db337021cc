"""Problem-iterations per second of the wide batch (totsu_amd.WideBatchSolver: one workgroup per problem, only the pass vectors in
LDS, every other vector worked on in place in the arena, A streamed from memory twice per iteration), eps_acc = 1e-30 so that nothing
stops, one process, every route timed twice:
  (a) against the only earlier route for its shapes -- sixteen FusedSolver(schedule="carried") one after the other (its rate does
      not depend on P) -- on feasible LPs over the nonnegative cone (the construction of tests/ownbatch_cases.py) at 2020 x 1000,
      3000 x 1500, 4096 x 2048 and 4096 x 4096, and on an SDP with one order-64 cone (random_sdp(200, 64): 2080 x 200);
  (b) against MidBatchSolver itself on LP 1024 x 512 and 2000 x 1000, where both take the shape: the price of the vectors in memory.
P = 16, 64, 256 and 1024 problems (a size whose A would not fit --mem-gb is left out and said so).  Host clock around run() with the
stream synchronised; construction, init and a warm-up run are outside the timed span on every route.  A timed window lasts about
--window seconds (the iteration count is scaled from a first short window).  No ratio is a condition: the figures are what they
are, losses included.  profiles/widebatch_rate.txt.
    python tools/widebatch_rate.py [--window 0.3] [--base-iters 64] [--poll 16] [--sizes 16,64,256,1024] [--mem-gb 150] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import totsu_amd as T  # noqa: E402
from problems import random_sdp  # noqa: E402
from totsu_amd import _lib  # noqa: E402
from totsu_amd._lib import lib  # noqa: E402

F = np.float32
DISTINCT = 4             # problems generated per family; larger P repeat them (every slot still streams its own copy of the data)
PEAK = 8.0e12            # bytes per second: the chip-wide figure the fractions refer to


def lp_family(m, n, k):
    """feasible LPs over the nonnegative cone (tests/ownbatch_cases.py::_edge): b = A x0 + s0, c = -A^T y0"""
    a, b, c = [], [], []
    for s in range(k):
        rng = np.random.default_rng(1000 * m + n + 7919 * s)
        A = (rng.standard_normal((m, n)) / np.sqrt(n)).astype(F)
        x0, s0, y0 = rng.standard_normal(n), rng.uniform(0.1, 1.1, m), rng.uniform(0.1, 1.1, m)
        a.append(np.asfortranarray(A).ravel(order="F"))
        b.append((A.astype(np.float64) @ x0 + s0).astype(F))
        c.append((-A.astype(np.float64).T @ y0).astype(F))
    return dict(name="LP %d x %d" % (m, n), n=n, m=m, a=np.stack(a), b=np.stack(b), c=np.stack(c), seg_type=[_lib.CONE_RPOS], seg_len=[m])


def sdp_family(n, order, k):
    a, b, c = [], [], []
    for s in range(k):
        cc, syms = random_sdp(n, order, seed=s)
        mb = lambda typ: T.MatBuild(T.F32HIP, typ)
        sdp = T.ProbSDP(mb(T.MatType.General(n, 1)).set_array(cc.reshape(-1, 1)), [mb(T.MatType.SymPack(order)).set_array(s_) for s_ in syms],
                        mb(T.MatType.General(0, n)), mb(T.MatType.General(0, 1)), 1e-12)
        d = sdp.dense()
        sdp.drop()
        a.append(np.asarray(d.mat_a, F).ravel())
        b.append(np.asarray(d.vec_b, F))
        c.append(np.asarray(d.vec_c, F))
        seg = (list(d.seg_type), list(d.seg_len))
    m = b[0].size
    return dict(name="SDP order %d, %d x %d" % (order, m, n), n=n, m=m, a=np.stack(a), b=np.stack(b), c=np.stack(c), seg_type=seg[0],
                seg_len=seg[1])


def timed(fn):
    lib.thip_sync()
    t0 = time.perf_counter()
    fn()
    lib.thip_sync()
    return time.perf_counter() - t0


def stacked(x, P):
    """P rows on the device, row p a copy of x[p % len(x)], uploaded row by row (the host never holds P copies)"""
    d = T.DeviceBuffer(P * x.shape[1])
    for p in range(P):
        row = np.ascontiguousarray(x[p % x.shape[0]], dtype=F)
        lib.thip_h2d(d.ptr + 4 * p * row.size, row.ctypes.data, row.size)
    return d


def compute_units():
    try:
        import torch
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    except Exception:
        return 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--base-iters", type=int, default=64)
    ap.add_argument("--poll", type=int, default=16)
    ap.add_argument("--sizes", default="16,64,256,1024")
    ap.add_argument("--mem-gb", type=float, default=150.0)
    ap.add_argument("--only", default="", help="comma-separated family indices (0 .. 6) to run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init()
    cus = compute_units()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    p = T.SolverParam()
    p.eps_acc = 1e-30
    say("widebatch_rate: problem-iterations per second, eps_acc = 1e-30 (nothing stops), poll_every = %d, %d CUs" % (a.poll, cus))
    say("   new: WideBatchSolver, windows of about %.2f s, every route timed twice (both figures given, the ratio is of the means)" % a.window)
    say("   (a) baseline: 16 x FusedSolver(\"carried\") in turn, %d iterations each;  (b) baseline: MidBatchSolver at the same P" % a.base_iters)
    say("   bytes of A: 2 m n 4 per problem-iteration; chip-wide, as a fraction of 8 TB/s, and per busy CU (min(P, CUs))")
    fams = [("a", lambda: lp_family(2020, 1000, DISTINCT)), ("a", lambda: lp_family(3000, 1500, DISTINCT)),
            ("a", lambda: lp_family(4096, 2048, DISTINCT)), ("a", lambda: lp_family(4096, 4096, DISTINCT)),
            ("a", lambda: sdp_family(200, 64, DISTINCT)),
            ("b", lambda: lp_family(1024, 512, DISTINCT)), ("b", lambda: lp_family(2000, 1000, DISTINCT))]
    only = [int(v) for v in a.only.split(",") if v]
    sizes = [int(v) for v in a.sizes.split(",")]
    summary = []

    def batch_rate(cls, fam, P):
        n, m = fam["n"], fam["m"]
        bufs = [stacked(fam[k], P) for k in ("a", "b", "c")]
        sb = cls(n, m, bufs[0], bufs[1], bufs[2], fam["seg_type"], fam["seg_len"], p)
        sb.run(a.poll, a.poll)                         # warm-up
        probe = a.poll
        iters = max(probe, int(probe * a.window / timed(lambda: sb.run(probe, a.poll))) // a.poll * a.poll)
        dts = [timed(lambda: sb.run(iters, a.poll)) for _ in range(2)]
        res = [sb.status(i) for i in (0, P - 1)]
        assert all(r.iters == a.poll + probe + 2 * iters and r.state == _lib.ST_RUNNING for r in res)
        info = sb.info()
        sb.destroy()
        for d in bufs:
            d.free()
        return [P * iters / dt for dt in dts], iters, info

    for idx, (part, make) in enumerate(fams):
        if only and idx not in only:
            continue
        fam = make()
        n, m = fam["n"], fam["m"]
        say()
        say("(%s) %s  (m * n = %d, %.2f MB of A read per problem-iteration)" % (part, fam["name"], m * n, 8 * m * n / 1e6))
        base = None
        if part == "a":
            k = fam["a"].shape[0]
            solvers = [T.FusedSolver(n, m, fam["a"][i % k], fam["b"][i % k], fam["c"][i % k], fam["seg_type"], fam["seg_len"], p, "carried")
                       for i in range(16)]
            for fs in solvers:
                fs.run(4, a.poll)                      # warm-up
            dts = [timed(lambda: [fs.run(a.base_iters, a.poll) for fs in solvers]) for _ in range(2)]
            assert all(fs.status().iters == 4 + 2 * a.base_iters for fs in solvers)
            for fs in solvers:
                fs.destroy()
            rates = [16 * a.base_iters / dt for dt in dts]
            base = sum(rates) / 2
            say("   baseline  16 FusedSolver(carried) in turn   %10.0f / %10.0f problem-iterations/s  (%.1f us per iteration)"
                % (rates[0], rates[1], 1e6 / base))
        lost = []
        for P in sizes:
            if 4.0 * m * n * P > a.mem_gb * 1e9:
                say("   P = %-5d left out: %.0f GB of A" % (P, 4.0 * m * n * P / 1e9))
                continue
            if part == "b":
                mr, mit, minfo = batch_rate(T.MidBatchSolver, fam, P)
                base = sum(mr) / 2
                say("   P = %-5d MidBatchSolver  %4d threads %6d B LDS %6d iterations %10.0f / %10.0f problem-iterations/s"
                    % (P, minfo["threads"], minfo["lds_bytes"], mit, mr[0], mr[1]))
            wr, it, info = batch_rate(T.WideBatchSolver, fam, P)
            rate = sum(wr) / 2
            bps = rate * info["a_bytes_per_iter"]
            say("   P = %-5d WideBatchSolver %4d threads %6d B LDS %6d iterations %10.0f / %10.0f problem-iterations/s  ratio %7.2f  "
                "A: %6.3f TB/s = %5.1f %% of 8 TB/s, %6.2f GB/s per busy CU"
                % (P, info["threads"], info["lds_bytes"], it, wr[0], wr[1], rate / base, bps / 1e12, 100.0 * bps / PEAK,
                   bps / 1e9 / min(P, cus)))
            if rate < base:
                lost.append(P)
            summary.append((part, fam["name"], P, rate / base))
        say("   the baseline wins at this shape %s" % ("at P = %s of the sizes run" % ", ".join(map(str, lost)) if lost else "at no size run"))
    say()
    say("ratios to the baseline: " + "; ".join("(%s) %s P=%d %.2f" % s for s in summary))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
