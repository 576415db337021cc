"""What streaming problems through the slots of a batch, and launches that follow the live set, gain on the 0.8 GB LP shape of
tools/batch_rate.py (m = 20 000, n = 10 000, seeded): 64 (b, c) drawn from the LP generator's distributions, solved to eps_acc over
the same A in four ways in one process --
    1. eight fixed batches of 8, one after the other (each repeats the |A| sums and the autotune, each ends in a tail of launches
       that serve few live instances)
    2. totsu_amd.solve_many with 8 slots (one batch, regroup=True, a slot refilled as soon as its problem has stopped)
    3. one fixed batch of 64
    4. one batch of 64 with regroup=True
-- wall time (construction, autotune and read-out included), problems / s, and the batch's counters: instance_iterations, passes
over A, launches by kernel instance.  profiles/batch_stream_rate.txt.
    python tools/batch_stream_rate.py [--n 10000] [--problems 64] [--eps 1e-2] [--max-iter 100000] [--poll 32] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import totsu_amd as T  # noqa: E402
from totsu_amd import _lib  # noqa: E402
from totsu_amd._lib import lib  # noqa: E402
from totsu_amd.synth import STREAM_C, STREAM_H, LpInstance, _gen  # noqa: E402


def add(total, c):
    for k in ("passes", "instance_iterations", "replaced"):
        total[k] = total.get(k, 0) + c[k]
    la = total.setdefault("launches", {1: 0, 2: 0, 4: 0, 8: 0})
    for nv, v in c["launches"].items():
        la[nv] += v
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--eps", type=float, default=1e-2)
    ap.add_argument("--max-iter", type=int, default=100000)
    ap.add_argument("--poll", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    inst = LpInstance(a.n, seed=0)
    m, n, P = inst.m, inst.n, a.problems
    dense = T.problem._Dense(n, m, inst.mat_a, None, None, inst.seg_type, inst.seg_len)
    say("batch_stream_rate: benchmark_lp shape m = %d, n = %d, A = %.3f GB f32; %d problems (b, c) from the generator's distributions"
        % (m, n, 4.0 * m * n / 1e9, P))
    say("   eps_acc = %g, max_iter = %d, poll_every = %d, autotune on; wall time by the host clock around construction, solve and read-out"
        % (a.eps, a.max_iter, a.poll))
    D = T.DeviceBuffer
    bs, cs = [], []
    for i in range(P):
        h = _gen(m, i, STREAM_H, 0, 0)
        h[:n] = 0.0
        bs.append(D.from_host(h))
        cs.append(D.from_host(-_gen(n, i, STREAM_C, 0, 0)))
    p = T.SolverParam()
    p.eps_acc, p.max_iter = a.eps, a.max_iter

    def fixed(idx, regroup):
        bt = T.BatchSolver.from_dense(dense, [bs[i] for i in idx], [cs[i] for i in idx], p, regroup=regroup)
        res = bt.run(-1, a.poll)
        xs = [bt.solution(i)[0] for i in range(len(idx))]
        c = bt.counters()
        bt.destroy()
        return [(r.state, r.iters) for r in res], xs, c

    def eight_of_eight():
        out, xs, tot = [], [], {}
        for g in range(0, P, 8):
            o, x, c = fixed(range(g, min(g + 8, P)), False)
            out, xs, tot = out + o, xs + x, add(tot, c)
        return out, xs, tot

    def streamed():
        out = T.solve_many(dense, bs, cs, slots=8, param=p, poll_every=a.poll)
        return [(r.state, r.iters) for r, _, _ in out], [x for _, x, _ in out], add({}, out.counters)

    variants = [("1. eight fixed batches of 8, in turn", eight_of_eight),
                ("2. solve_many, 8 slots", streamed),
                ("3. one fixed batch of %d" % min(P, 64), lambda: (lambda o: (o[0], o[1], add({}, o[2])))(fixed(range(min(P, 64)), False))),
                ("4. one batch of %d, regroup" % min(P, 64), lambda: (lambda o: (o[0], o[1], add({}, o[2])))(fixed(range(min(P, 64)), True)))]
    fixed(range(min(P, 2)), False)                       # warm-up: code objects loaded, clocks up
    say()
    say("   %-38s %9s %11s %14s %9s   %s" % ("", "wall s", "problems/s", "inst-iterations", "passes", "launches {1, NV=2, 4, 8}"))
    ref = None
    for name, fn in variants:
        lib.thip_sync()
        t0 = time.perf_counter()
        out, xs, c = fn()
        lib.thip_sync()
        dt = time.perf_counter() - t0
        say("   %-38s %9.2f %11.2f %14d %9d   %s" % (name, dt, len(out) / dt, c["instance_iterations"], c["passes"],
                                                    [c["launches"][nv] for nv in (1, 2, 4, 8)]))
        if ref is None:
            ref = (out, xs)
            it = np.array([o[1] for o in out])
            say("       iterations per problem: min %d, median %d, max %d; states %s" % (it.min(), np.median(it), it.max(),
                                                                                       sorted(set(o[0] for o in out))))
        else:                                            # the same problems solved: states, and how far iteration counts and x moved
            same = sum(o[0] == r[0] for o, r in zip(out, ref[0]))
            dit = max(abs(o[1] - r[1]) for o, r in zip(out, ref[0]))
            dx = max(float(np.abs(x - rx).max()) for x, rx in zip(xs, ref[1]))
            say("       against 1.: %d of %d states equal, iteration counts differ by at most %d, max |x - x'| = %.2e" % (same, len(out), dit, dx))
    for b in bs + cs:
        b.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
