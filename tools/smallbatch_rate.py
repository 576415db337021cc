"""Problem-iterations per second of the on-chip small batch (totsu_amd.SmallBatchSolver, one workgroup per problem, A in LDS) on
the 80 x 40 LP family (benchmark_lp(40)) and the 102 x 12 SOCP family (random_socp(12, [5, 1, 0, 17, 70, 3])) at P = 64, 256, 1024
and 4096 problems, eps_acc = 1e-30 so that nothing stops -- against the only other route for problems that each have their own A:
one FusedSolver(schedule="carried") per problem, one after the other (sixteen problems of the family: its rate does not depend on P),
in the same process on the same device.  Host clock around run() with the stream synchronised; construction, init and a warm-up
run are outside the timed span on both sides.  A timed window lasts about --window seconds (the iteration count is scaled from a
first short window) and is taken three times: the median is reported, with the spread.  profiles/smallbatch_rate.txt.
    python tools/smallbatch_rate.py [--window 0.5] [--base-iters 1024] [--poll 64] [--sizes 64,256,1024,4096] [--out FILE]"""
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
DISTINCT = 64            # problems generated per family; larger P repeat them (every slot still iterates its own copy of the data)


def lp_family(k):
    a, b, c = [], [], []
    for s in range(k):
        cc, G, h = benchmark_lp(40, seed=s)
        a.append(np.asfortranarray(G).ravel(order="F"))
        b.append(h)
        c.append(cc)
    return dict(name="LP 80 x 40", n=40, m=80, a=np.stack(a), b=np.stack(b), c=np.stack(c), rowabs=None,
                seg_type=[_lib.CONE_RPOS], seg_len=[80])


def socp_family(k):
    n, cones = 12, [5, 1, 0, 17, 70, 3]
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
    return dict(name="SOCP 102 x 12", n=n, m=a[0].size // n, a=np.stack(a), b=np.stack(b), c=np.stack(c), rowabs=np.stack(ra),
                seg_type=[_lib.CONE_SOC] * len(cones), seg_len=[1 + k_ for k_ in cones])


def timed(fn):
    lib.thip_sync()
    t0 = time.perf_counter()
    fn()
    lib.thip_sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--base-iters", type=int, default=1024)
    ap.add_argument("--poll", type=int, default=64)
    ap.add_argument("--sizes", default="64,256,1024,4096")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    p = T.SolverParam()
    p.eps_acc = 1e-30
    say("smallbatch_rate: problem-iterations per second, eps_acc = 1e-30 (nothing stops), poll_every = %d" % a.poll)
    say("   new: SmallBatchSolver, windows of about %.2f s; baseline: 16 x FusedSolver(\"carried\") in turn, %d iterations each; median of 3 windows"
        % (a.window, a.base_iters))
    ok = True
    for fam in (lp_family(DISTINCT), socp_family(DISTINCT)):
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
        say("%s  (m * n = %d)" % (fam["name"], m * n))
        say("   baseline  16 solvers in turn          %8.3f s (%.3f .. %.3f)  %12.0f problem-iterations/s  (%.1f us per iteration)"
            % (dt, dts[0], dts[2], base, 1e6 / base))
        for P in [int(v) for v in a.sizes.split(",")]:
            rep = (P + DISTINCT - 1) // DISTINCT
            tile = lambda x: None if x is None else np.tile(x, (rep, 1))[:P]
            sb = T.SmallBatchSolver(n, m, tile(fam["a"]), tile(fam["b"]), tile(fam["c"]), fam["seg_type"], fam["seg_len"], p,
                                    vecs_b_rowabs=tile(fam["rowabs"]))
            sb.run(8, a.poll)                          # warm-up
            probe = 8 * a.poll
            iters = max(probe, int(probe * a.window / timed(lambda: sb.run(probe, a.poll))) // a.poll * a.poll)
            dts = sorted(timed(lambda: sb.run(iters, a.poll)) for _ in range(3))
            res = [sb.status(i) for i in (0, P - 1)]
            assert all(r.iters == 8 + probe + 3 * iters and r.state == _lib.ST_RUNNING for r in res)
            info = sb.info()
            sb.destroy()
            dt = dts[1]
            rate = P * iters / dt
            say("   P = %-5d %4d threads %6d B LDS  %7d iterations  %8.3f s (%.3f .. %.3f)  %12.0f problem-iterations/s  ratio to baseline %8.1f"
                % (P, info["threads"], info["lds_bytes"], iters, dt, dts[0], dts[2], rate, rate / base))
            if P == 256:
                verdict = rate / base >= 16.0
                ok = ok and verdict
                say("      condition at P = 256 (ratio >= 16): %s" % ("met" if verdict else "NOT met"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
