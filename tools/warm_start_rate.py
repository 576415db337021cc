"""What a start iterate saves on two families of related problems, measured, with no figure promised in advance: how much a start
saves is a property of the path.  One process, eps_acc = 1e-3, every route run twice.
    (a) shared A: a path of 32 LPs on the 2504 x 1252 benchmark_lp shape, c_k = c (1 + lambda_k w) (w ~ U(0, 1), every c_k < 0 as
        benchmark_lp's c is), through totsu_amd.solve_many(slots=8) cold and with warm=True -- total instance-iterations, wall time
        and passes over A
    (b) own A: MidBatchSolver, benchmark_lp 256 x 128 per problem, P = 256, eight rounds with b perturbed by 1 % per round; every
        slot refilled by replace cold against replace(start=raw_iterate) -- total problem-iterations to stop and wall time; and the
        time of one set_iterates over all P beside one reinit
profiles/warm_start.txt.
    python tools/warm_start_rate.py [--path 32] [--prob 256] [--rounds 8] [--eps 1e-3] [--max-iter 200000] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import totsu_amd as T  # noqa: E402
from totsu_amd import _lib  # noqa: E402
from totsu_amd._lib import lib  # noqa: E402

F = np.float32


def benchmark_lp(sz, seed):
    """experimental/benchmark_lp: n = sz, m = 2 sz, c = -U(0, 1), G = [-I; U(0, 1)], h = [0; U(0, 1)]"""
    rng = np.random.default_rng(seed)
    c = -rng.uniform(0, 1, sz)
    G = np.vstack([-np.eye(sz), rng.uniform(0, 1, (sz, sz))])
    h = np.concatenate([np.zeros(sz), rng.uniform(0, 1, sz)])
    return c.astype(F), G.astype(F), h.astype(F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", type=int, default=32)
    ap.add_argument("--prob", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--max-iter", type=int, default=200000)
    ap.add_argument("--poll", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    p = T.SolverParam()
    p.eps_acc, p.max_iter = a.eps, a.max_iter
    say("warm_start_rate: eps_acc = %g, max_iter = %d, poll_every = %d; wall time by the host clock around construction, solve and read-out"
        % (a.eps, a.max_iter, a.poll))

    # ---- (a) a path over a shared A -------------------------------------------------------------------------------------------
    c, G, h = benchmark_lp(1252, 0)
    m, n = G.shape
    dense = T.problem._Dense(n, m, T.DeviceBuffer.from_host(np.asfortranarray(G).ravel(order="F")), None, None, [_lib.CONE_RPOS], [m])
    w = np.random.default_rng(5).uniform(0, 1, n)
    cs = [(c * (1 + 0.01 * k * w)).astype(F) for k in range(a.path)]
    bs = [h] * a.path
    say()
    say("(a) shared A: a path of %d LPs, %d x %d, c_k = c (1 + 0.01 k w); solve_many(slots=8)" % (a.path, m, n))
    say("   %-22s %9s %16s %9s %9s   %s" % ("", "wall s", "inst-iterations", "passes", "replaced", "states"))
    T.solve_many(dense, bs[:2], cs[:2], slots=2, param=p, poll_every=a.poll)          # warm-up: code objects loaded, clocks up
    ref = None
    for rep in range(2):
        for warm in (False, True):
            lib.thip_sync()
            t0 = time.perf_counter()
            out = T.solve_many(dense, bs, cs, slots=8, param=p, poll_every=a.poll, warm=warm)
            lib.thip_sync()
            dt = time.perf_counter() - t0
            ct = out.counters
            say("   %-22s %9.3f %16d %9d %9d   %s" % ("%s, run %d" % ("warm=True" if warm else "cold", rep + 1), dt, ct["instance_iterations"],
                                                      ct["passes"], ct["replaced"], sorted(set(r.state for r, _, _ in out))))
            xs = [x for _, x, _ in out]
            if ref is None:
                ref = xs
            else:
                say("       against the first cold run: max |x - x'| / max(1, |x|) = %.2e"
                    % max(float(np.abs(x - r).max() / max(1.0, np.abs(r).max())) for x, r in zip(xs, ref)))
    dense.mat_a.free()

    # ---- (b) rounds of perturbed b over own A ---------------------------------------------------------------------------------
    P = a.prob
    lps = [benchmark_lp(128, 1000 + q) for q in range(P)]
    mats = np.stack([np.asfortranarray(g).ravel(order="F") for _, g, _ in lps])
    b0 = np.stack([hh for _, _, hh in lps])
    c0 = np.stack([cc for cc, _, _ in lps])
    rng = np.random.default_rng(11)
    rounds = [b0]
    for _ in range(a.rounds):
        rounds.append((rounds[-1] * (1 + 0.01 * rng.standard_normal(b0.shape))).astype(F))
    say()
    say("(b) own A: MidBatchSolver, benchmark_lp 256 x 128 per problem, P = %d, %d rounds, b perturbed by 1 %% per round; every slot"
        % (P, a.rounds))
    say("    refilled by replace each round (the first solve, from zero, is not counted)")
    say("   %-22s %9s %18s   %s" % ("", "wall s", "problem-iterations", "states"))
    for rep in range(2):
        for warm in (False, True):
            sb = T.MidBatchSolver(128, 256, mats, rounds[0], c0, [_lib.CONE_RPOS], [256], p)
            sb.run(-1, a.poll)
            lib.thip_sync()
            t0 = time.perf_counter()
            total, states = 0, set()
            for r in range(1, a.rounds + 1):
                for i in range(P):
                    start = sb.raw_iterate(i) if warm else None
                    sb.replace(i, mats[i], rounds[r][i], c0[i], start=start)
                res = sb.run(-1, a.poll)
                total += sum(q.iters + 1 for q in res)
                states |= set(q.state for q in res)
            lib.thip_sync()
            dt = time.perf_counter() - t0
            say("   %-22s %9.3f %18d   %s" % ("%s, run %d" % ("replace(start=raw)" if warm else "replace cold", rep + 1), dt, total, sorted(states)))
            if rep == 1 and warm:
                its = [sb.raw_iterate(i) for i in range(P)]
                xs, ys = [x for x, _ in its], [y for _, y in its]
                for what, fn in (("one set_iterates over all %d" % P, lambda: sb.set_iterates(xs, ys)), ("one reinit", sb.reinit)):
                    best = 1e30
                    for _ in range(5):
                        lib.thip_sync()
                        t0 = time.perf_counter()
                        fn()
                        lib.thip_sync()
                        best = min(best, time.perf_counter() - t0)
                    say("   %-32s %9.1f us (best of 5; the host's packing and the upload included)" % (what, 1e6 * best))
            sb.destroy()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
