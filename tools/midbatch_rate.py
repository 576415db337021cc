"""Problem-iterations per second of the streamed mid-size batch (totsu_amd.MidBatchSolver, one workgroup per problem, the vectors in
LDS, A streamed from memory twice per iteration) on the LP family benchmark_lp(n) (m = 2 n) at n = 128, 256, 512, 1000 and on the
423 x 60 SOCP family random_socp(60, [5, 1, 0, 17, 140, 250, 3]) at P = 16, 64, 256 and 1024 problems, eps_acc = 1e-30 so that nothing
stops -- against the only other route for such problems: one FusedSolver(schedule="carried") per problem, one after the other
(sixteen problems of the family: its rate does not depend on P), in the same process on the same device.  Host clock around run()
with the stream synchronised; construction, init and a warm-up run are outside the timed span on both sides.  A timed window lasts
about --window seconds (the iteration count is scaled from a first short window) and is taken three times: the median is reported,
with the spread.  Beside the rate: the bytes of A read per second (2 m n 4 per problem-iteration) chip-wide, as a fraction of 8 TB/s,
and per busy CU (min(P, CUs)).  No ratio is a condition: the figures are what they are.  profiles/midbatch_rate.txt.
    python tools/midbatch_rate.py [--window 0.3] [--base-iters 512] [--poll 32] [--sizes 16,64,256,1024] [--lp 128,256,512,1000] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import totsu_amd as T  # noqa: E402
from problems import benchmark_lp, random_socp  # noqa: E402
from totsu_amd import _lib  # noqa: E402
from totsu_amd._lib import lib  # noqa: E402

F = np.float32
DISTINCT = 16            # problems generated per family; larger P repeat them (every slot still streams its own copy of the data)
PEAK = 8.0e12            # bytes per second: the chip-wide figure the fractions refer to


def lp_family(sz, k):
    a, b, c = [], [], []
    for s in range(k):
        cc, G, h = benchmark_lp(sz, seed=s)
        a.append(np.asfortranarray(G).ravel(order="F"))
        b.append(h)
        c.append(cc)
    return dict(name="LP %d x %d" % (2 * sz, sz), n=sz, m=2 * sz, a=np.stack(a), b=np.stack(b), c=np.stack(c), rowabs=None,
                seg_type=[_lib.CONE_RPOS], seg_len=[2 * sz])


def socp_family(k):
    n, cones = 60, [5, 1, 0, 17, 140, 250, 3]
    a, b, c, ra = [], [], [], []
    for s in range(k):
        f, Gs, hs, cs, d = random_socp(n, cones, seed=s)
        rows, bs, babs = [], [], []
        for G, h, ci, di in zip(Gs, hs, cs, d):        # ProbSOCP.dense(): rows of cone i are [-c_i^T ; -G_i], b = [d_i ; h_i]
            rows += [-ci.reshape(1, n), -G]
            bs += [np.array([di], F), h]
            babs += [np.array([di], F), np.abs(h)]
        A = np.vstack(rows).astype(F)
        a.append(np.asfortranarray(A).ravel(order="F"))
        b.append(np.concatenate(bs).astype(F))
        ra.append(np.concatenate(babs).astype(F))
        c.append(f)
    m = a[0].size // n
    return dict(name="SOCP %d x %d" % (m, n), n=n, m=m, a=np.stack(a), b=np.stack(b), c=np.stack(c), rowabs=np.stack(ra),
                seg_type=[_lib.CONE_SOC] * len(cones), seg_len=[1 + k_ for k_ in cones])


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
    ap.add_argument("--base-iters", type=int, default=512)
    ap.add_argument("--poll", type=int, default=32)
    ap.add_argument("--sizes", default="16,64,256,1024")
    ap.add_argument("--lp", default="128,256,512,1000")
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
    say("midbatch_rate: problem-iterations per second, eps_acc = 1e-30 (nothing stops), poll_every = %d, %d CUs" % (a.poll, cus))
    say("   new: MidBatchSolver, windows of about %.2f s; baseline: 16 x FusedSolver(\"carried\") in turn, %d iterations each; median of 3 windows"
        % (a.window, a.base_iters))
    say("   bytes of A: 2 m n 4 per problem-iteration; chip-wide, as a fraction of 8 TB/s, and per busy CU (min(P, CUs))")
    fams = [lambda sz=int(v): lp_family(sz, DISTINCT) for v in a.lp.split(",") if v] + [lambda: socp_family(DISTINCT)]
    summary = []
    for make in fams:
        fam = make()
        n, m = fam["n"], fam["m"]
        # the baseline: what a caller with one A per problem could do before -- a solver per problem, in turn
        solvers = [T.FusedSolver(n, m, fam["a"][i], fam["b"][i], fam["c"][i], fam["seg_type"], fam["seg_len"], p, "carried",
                                 vec_b_rowabs=None if fam["rowabs"] is None else fam["rowabs"][i]) for i in range(16)]
        for fs in solvers:
            fs.run(8, a.poll)                          # warm-up
        dts = sorted(timed(lambda: [fs.run(a.base_iters, a.poll) for fs in solvers]) for _ in range(3))
        assert all(fs.status().iters == 8 + 3 * a.base_iters for fs in solvers)
        for fs in solvers:
            fs.destroy()
        dt = dts[1]
        base = 16 * a.base_iters / dt
        say()
        say("%s  (m * n = %d, %.2f MB of A read per problem-iteration)" % (fam["name"], m * n, 8 * m * n / 1e6))
        say("   baseline  16 solvers in turn                 %8.3f s (%.3f .. %.3f)  %10.0f problem-iterations/s  (%.1f us per iteration)"
            % (dt, dts[0], dts[2], base, 1e6 / base))
        crossover = None
        for P in [int(v) for v in a.sizes.split(",")]:
            bufs = [stacked(fam[k], P) for k in ("a", "b", "c")] + ([] if fam["rowabs"] is None else [stacked(fam["rowabs"], P)])
            sb = T.MidBatchSolver(n, m, bufs[0], bufs[1], bufs[2], fam["seg_type"], fam["seg_len"], p,
                                  vecs_b_rowabs=bufs[3] if len(bufs) > 3 else None)
            sb.run(8, a.poll)                          # warm-up
            probe = 2 * a.poll
            iters = max(probe, int(probe * a.window / timed(lambda: sb.run(probe, a.poll))) // a.poll * a.poll)
            dts = sorted(timed(lambda: sb.run(iters, a.poll)) for _ in range(3))
            res = [sb.status(i) for i in (0, P - 1)]
            assert all(r.iters == 8 + probe + 3 * iters and r.state == _lib.ST_RUNNING for r in res)
            info = sb.info()
            sb.destroy()
            for d in bufs:
                d.free()
            dt = dts[1]
            rate = P * iters / dt
            bps = rate * info["a_bytes_per_iter"]
            say("   P = %-5d %4d threads %6d B LDS %2d-byte loads %6d iterations %7.3f s (%.3f .. %.3f) %10.0f problem-iterations/s  "
                "ratio %7.2f  A: %6.3f TB/s = %5.1f %% of 8 TB/s, %6.2f GB/s per busy CU"
                % (P, info["threads"], info["lds_bytes"], info["load_bytes"], iters, dt, dts[0], dts[2], rate, rate / base, bps / 1e12,
                   100.0 * bps / PEAK, bps / 1e9 / min(P, cus)))
            if rate < base:
                crossover = P
            summary.append((fam["name"], P, rate / base))
        say("   the baseline wins at this shape %s" % ("up to P = %d of the sizes run" % crossover if crossover else "at no size run"))
    say()
    say("ratios to the baseline: " + "; ".join("%s P=%d %.2f" % s for s in summary))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
