"""Problem-iterations per second of the wide batch over a 16-bit copy of A (totsu_amd.Wide16BatchSolver, a_dtype "bf16" and "f16")
against the f32 wide batch (totsu_amd.WideBatchSolver) on the same problems in the same run: tools/widebatch_rate.py's protocol -- one
process, eps_acc = 1e-30 so that nothing stops, construction, init and a warm-up run outside the timed span, the host clock around
run() with the stream synchronised -- on its families: feasible LPs over the nonnegative cone at 2020 x 1000, 3000 x 1500,
4096 x 2048 and 4096 x 4096, and the SDP with one order-64 cone (2080 x 200), at P = 16, 64 and 256.
Every route is run TWICE (the same handle, two windows of about --window seconds each); both rates are printed, the ratio is of the
means and the spread is the two runs' distance.  Every step runs under a time limit of its own (--step-limit seconds, an alarm): a
step that overruns ends the tool, which starts nothing more.  Beside the rate: the bytes of A read per second (info()'s
a_bytes_per_iter per problem-iteration) and the device memory of the route -- the handle's own (info()'s device_bytes: for a 16-bit
route the store included) and, for f32, the caller's stack of A that the handle reads in place.
The f32 stack of a (shape, P) is uploaded once: the f32 handle reads it, each 16-bit handle converts from it and keeps no reference.
No ratio is a condition; every (shape, P) where a 16-bit route is slower is listed as plainly as the wins.
profiles/wide16batch_rate.txt.
    python tools/wide16batch_rate.py [--window 0.3] [--poll 16] [--sizes 16,64,256] [--only 0,1,2,3,4] [--out FILE]"""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import totsu_amd as T  # noqa: E402
from mid16batch_rate import StepLimit, limited  # noqa: E402
from totsu_amd import _lib  # noqa: E402
from widebatch_rate import PEAK, lp_family, sdp_family, stacked, timed  # noqa: E402

DISTINCT = 4             # problems generated per family; larger P repeat them (every slot still streams its own copy of the data)
ROUTES = ("f32", "bf16", "f16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--poll", type=int, default=16)
    ap.add_argument("--sizes", default="16,64,256")
    ap.add_argument("--mem-gb", type=float, default=150.0)
    ap.add_argument("--step-limit", type=float, default=120.0)
    ap.add_argument("--only", default="", help="comma-separated family indices (0 .. 4) to run")
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
    say("wide16batch_rate: problem-iterations per second, eps_acc = 1e-30 (nothing stops), poll_every = %d; one process" % a.poll)
    say("   routes: WideBatchSolver (f32), Wide16BatchSolver bf16 and f16, the same problems; every route twice, windows of about %.2f s,"
        % a.window)
    say("   each step under a limit of %.0f s; ratio: mean rate over the f32 mean; spread: |run 1 - run 2| / mean" % a.step_limit)
    say("   memory: the handle's device_bytes (16-bit: the store included); f32: and the caller's stack of A, which it reads in place")
    fams = [lambda: lp_family(2020, 1000, DISTINCT), lambda: lp_family(3000, 1500, DISTINCT), lambda: lp_family(4096, 2048, DISTINCT),
            lambda: lp_family(4096, 4096, DISTINCT), lambda: sdp_family(200, 64, DISTINCT)]
    only = [int(v) for v in a.only.split(",") if v]
    summary = []

    def rate_of(route, fam, P, bufs):
        n, m = fam["n"], fam["m"]
        if route == "f32":
            sb = T.WideBatchSolver(n, m, bufs[0], bufs[1], bufs[2], fam["seg_type"], fam["seg_len"], p)
        else:
            sb = T.Wide16BatchSolver(n, m, bufs[0], bufs[1], bufs[2], fam["seg_type"], fam["seg_len"], p, a_dtype=route)
        try:
            limited(a.step_limit, lambda: sb.run(a.poll, a.poll))              # warm-up
            probe = a.poll
            t = limited(a.step_limit, lambda: timed(lambda: sb.run(probe, a.poll)))
            iters = max(probe, int(probe * a.window / t) // a.poll * a.poll)
            dts = [limited(a.step_limit, lambda: timed(lambda: sb.run(iters, a.poll))) for _ in range(2)]
            res = [sb.status(i) for i in (0, P - 1)]
            assert all(r.iters == a.poll + probe + 2 * iters and r.state == _lib.ST_RUNNING for r in res)
            return [P * iters / dt for dt in dts], iters, sb.info()
        finally:
            sb.destroy()

    try:
        for idx, mk in enumerate(fams):
            if only and idx not in only:
                continue
            fam = mk()
            n, m = fam["n"], fam["m"]
            say()
            say("%s  (f32: %.2f MB of A read per problem-iteration, %.2f MB of A held per problem)" % (fam["name"], 8 * m * n / 1e6, 4 * m * n / 1e6))
            for P in [int(v) for v in a.sizes.split(",")]:
                if 6.0 * m * n * P > a.mem_gb * 1e9:
                    say("   P = %-5d left out: %.0f GB of A (the f32 stack and a store)" % (P, 6.0 * m * n * P / 1e9))
                    continue
                bufs = limited(4 * a.step_limit, lambda: [stacked(fam[k], P) for k in ("a", "b", "c")])
                try:
                    base = None
                    for route in ROUTES:
                        rates, iters, info = rate_of(route, fam, P, bufs)
                        mean = sum(rates) / 2
                        spread = abs(rates[0] - rates[1]) / mean
                        if route == "f32":
                            base = mean
                        bps = mean * info["a_bytes_per_iter"]
                        mem = info["device_bytes"] + (4 * m * n * P if route == "f32" else 0)
                        say("   P = %-4d %-4s %4d threads %2d-byte loads %6d iterations  %9.0f / %9.0f problem-iterations/s  spread %5.2f %%  "
                            "A: %6.3f TB/s = %5.1f %% of 8 TB/s  memory %8.1f MB  ratio to f32 %5.2f"
                            % (P, route, info["threads"], info["load_bytes"], iters, rates[0], rates[1], 100 * spread, bps / 1e12,
                               100.0 * bps / PEAK, mem / 1e6, mean / base))
                        if route != "f32":
                            summary.append((fam["name"], P, route, mean / base, spread))
                        flush()
                finally:
                    for d in bufs:
                        d.free()
        say()
        say("ratios to f32 (spread of the 16-bit route's two runs): "
            + "; ".join("%s P=%d %s %.2f (%.1f %%)" % (s[0], s[1], s[2], s[3], 100 * s[4]) for s in summary))
        slower = ["%s P=%d %s %.2f" % s[:4] for s in summary if s[3] < 1.0]
        say("the 16-bit route is SLOWER than f32 at: " + ("; ".join(slower) if slower else "no (shape, P) run"))
    except StepLimit:
        say("a step overran its limit of %.0f s: nothing more was started" % a.step_limit)
        flush()
        return 1
    flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
