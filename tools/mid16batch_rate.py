"""Problem-iterations per second of the mid batch over a 16-bit copy of A (totsu_amd.Mid16BatchSolver, a_dtype "bf16" and "f16") against
the f32 mid batch (totsu_amd.MidBatchSolver) on the same problems: tools/midbatch_rate.py's protocol -- one process, eps_acc = 1e-30 so
that nothing stops, construction, init and a warm-up run outside the timed span, the host clock around run() with the stream
synchronised -- on its families: LP 256 x 128, 512 x 256, 1024 x 512, 2000 x 1000 and SOCP 423 x 60 at P = 16, 64, 256 and 1024.
Every route is run TWICE (the same handle, two windows of about --window seconds each); both rates are printed, the ratio is of the
means and the spread is the two runs' distance.  Every step runs under a time limit of its own (--step-limit seconds, an alarm): a
step that overruns ends the tool, which starts nothing more.  Beside the rate: the bytes of A read per second (info()'s
a_bytes_per_iter per problem-iteration).
Then the mixed route on LP 512 x 256 at P = 256, eps_acc = 1e-3: a 16-bit batch to its own stop, its raw iterates handed to an f32
batch on the exact matrix (set_iterates), against the f32 batch cold: wall time and problem-iterations of each.
No ratio is a condition.  profiles/mid16batch_rate.txt.
    python tools/mid16batch_rate.py [--window 0.3] [--poll 32] [--sizes 16,64,256,1024] [--lp 128,256,512,1000] [--out FILE]"""
import argparse
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import totsu_amd as T  # noqa: E402
from midbatch_rate import lp_family, socp_family, stacked, timed  # noqa: E402
from totsu_amd import _lib  # noqa: E402

DISTINCT = 16
PEAK = 8.0e12


class StepLimit(Exception):
    pass


def limited(seconds, fn):
    """fn() under an alarm of its own"""
    def ring(*_):
        raise StepLimit()
    old = signal.signal(signal.SIGALRM, ring)
    signal.alarm(int(seconds))
    try:
        return fn()
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def make(route, fam, P, p):
    """the route's batch over P problems of the family (the f32 stack of a 16-bit route is freed once the batch stands)"""
    n, m = fam["n"], fam["m"]
    bufs = [stacked(fam[k], P) for k in ("a", "b", "c")] + ([] if fam["rowabs"] is None else [stacked(fam["rowabs"], P)])
    kw = dict(vecs_b_rowabs=bufs[3] if len(bufs) > 3 else None)
    if route == "f32":
        sb = T.MidBatchSolver(n, m, bufs[0], bufs[1], bufs[2], fam["seg_type"], fam["seg_len"], p, **kw)
        return sb, bufs
    sb = T.Mid16BatchSolver(n, m, bufs[0], bufs[1], bufs[2], fam["seg_type"], fam["seg_len"], p, a_dtype=route, **kw)
    bufs[0].free()
    return sb, bufs[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--poll", type=int, default=32)
    ap.add_argument("--sizes", default="16,64,256,1024")
    ap.add_argument("--lp", default="128,256,512,1000")
    ap.add_argument("--step-limit", type=float, default=60.0)
    ap.add_argument("--no-mixed", action="store_true")
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
    say("mid16batch_rate: problem-iterations per second, eps_acc = 1e-30 (nothing stops), poll_every = %d; one process" % a.poll)
    say("   routes: MidBatchSolver (f32), Mid16BatchSolver bf16 and f16, the same problems; every route twice, windows of about %.2f s,"
        % a.window)
    say("   each step under a limit of %.0f s; ratio: mean rate over the f32 mean; spread: |run 1 - run 2| / mean" % a.step_limit)
    fams = [lambda sz=int(v): lp_family(sz, DISTINCT) for v in a.lp.split(",") if v] + [lambda: socp_family(DISTINCT)]
    summary = []
    try:
        for mk in fams:
            fam = mk()
            n, m = fam["n"], fam["m"]
            say()
            say("%s  (f32: %.3f MB of A per problem-iteration)" % (fam["name"], 8 * m * n / 1e6))
            for P in [int(v) for v in a.sizes.split(",")]:
                base = None
                for route in ("f32", "bf16", "f16"):
                    sb, bufs = limited(a.step_limit, lambda: make(route, fam, P, p))
                    limited(a.step_limit, lambda: sb.run(8, a.poll))          # warm-up
                    probe = 2 * a.poll
                    t = limited(a.step_limit, lambda: timed(lambda: sb.run(probe, a.poll)))
                    iters = max(probe, int(probe * a.window / t) // a.poll * a.poll)
                    dts = [limited(a.step_limit, lambda: timed(lambda: sb.run(iters, a.poll))) for _ in range(2)]
                    res = [sb.status(i) for i in (0, P - 1)]
                    assert all(r.iters == 8 + probe + 2 * iters and r.state == _lib.ST_RUNNING for r in res)
                    info = sb.info()
                    sb.destroy()
                    for d in bufs:
                        d.free()
                    rates = [P * iters / dt for dt in dts]
                    mean = sum(rates) / 2
                    spread = abs(rates[0] - rates[1]) / mean
                    if route == "f32":
                        base = mean
                    bps = mean * info["a_bytes_per_iter"]
                    say("   P = %-5d %-4s %4d threads %2d-byte loads %6d iterations  %10.0f / %10.0f problem-iterations/s  spread %5.2f %%  "
                        "A: %6.3f TB/s = %5.1f %% of 8 TB/s  ratio to f32 %5.2f"
                        % (P, route, info["threads"], info["load_bytes"], iters, rates[0], rates[1], 100 * spread, bps / 1e12,
                           100.0 * bps / PEAK, mean / base))
                    if route != "f32":
                        summary.append((fam["name"], P, route, mean / base, spread))
                    flush()
        say()
        say("ratios to f32 (spread of the 16-bit route's two runs): "
            + "; ".join("%s P=%d %s %.2f (%.1f %%)" % (s[0], s[1], s[2], s[3], 100 * s[4]) for s in summary))
        if not a.no_mixed:
            mixed(a, say)
    except StepLimit:
        say("a step overran its limit of %.0f s: nothing more was started" % a.step_limit)
        flush()
        return 1
    flush()
    return 0


def mixed(a, say):
    """16-bit to eps_acc = 1e-3, then f32 from its iterate, against f32 cold: LP 512 x 256, P = 256"""
    fam = lp_family(256, DISTINCT)
    P = 256
    p = T.SolverParam()
    p.eps_acc, p.max_iter = 1e-3, 200000
    say()
    say("the mixed route, %s, P = %d, eps_acc = 1e-3, poll_every = %d: wall seconds and problem-iterations" % (fam["name"], P, a.poll))

    def total(res):
        return sum(r.iters + 1 for r in res), sorted(set(r.state for r in res))

    f32, bufs = limited(a.step_limit, lambda: make("f32", fam, P, p))
    for rep in range(2):
        f32.reinit()
        t = limited(4 * a.step_limit, lambda: timed(lambda: f32.run(-1, a.poll)))
        its, states = total(f32.statuses())
        say("   cold f32, run %d:               %7.3f s  %9d problem-iterations  states %s" % (rep + 1, t, its, states))
    for route in ("bf16", "f16"):
        sb, b16 = limited(a.step_limit, lambda: make(route, fam, P, p))
        for rep in range(2):
            sb.reinit()
            f32.reinit()
            t16 = limited(4 * a.step_limit, lambda: timed(lambda: sb.run(-1, a.poll)))
            i16, s16 = total(sb.statuses())
            t0 = time.perf_counter()
            xs, ys = zip(*[sb.raw_iterate(i) for i in range(P)])
            f32.set_iterates(xs, ys)
            thand = time.perf_counter() - t0
            t32 = limited(4 * a.step_limit, lambda: timed(lambda: f32.run(-1, a.poll)))
            i32, s32 = total(f32.statuses())
            say("   %-4s then f32, run %d: %7.3f s + hand-over %6.3f s + %7.3f s = %7.3f s  %9d + %9d problem-iterations  states %s / %s"
                % (route, rep + 1, t16, thand, t32, t16 + thand + t32, i16, i32, s16, s32))
        sb.destroy()
        for d in b16:
            d.free()
    f32.destroy()
    for d in bufs:
        d.free()


if __name__ == "__main__":
    sys.exit(main())
