"""What a batch of problems that share A gains on the 0.8 GB LP shape (m = 20 000, n = 10 000, seeded): the multi-vector dual GEMV
(thip_gemv_multi.hip) against the single-vector dual_gemv_k on the same matrix, and instance-iterations per second of
totsu_amd.BatchSolver against one FusedSolver(schedule="carried"), all in one process.  Both as a fraction of 8 TB/s on the 4 m n bytes
of one pass.  profiles/batch_rate.txt.
    python tools/batch_rate.py [--n 10000] [--steps 300] [--rounds 3] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import totsu_amd as T  # noqa: E402
from totsu_amd import _lib  # noqa: E402
from totsu_amd._lib import lib  # noqa: E402
from totsu_amd.synth import STREAM_C, STREAM_H, LpInstance, _gen  # noqa: E402

PEAK = 8.0e12      # bytes / s


def ptrs(bufs):
    return (C.c_void_p * len(bufs))(*[b.ptr for b in bufs])


def kernel_ms(inst, nv, nj, blocks, xn, xt, on, ot, reps):
    ms = C.c_float()
    lib.thip_test_gemv_multi(inst.m, inst.n, inst.mat_a.ptr, nv, ptrs(xn[:nv]), ptrs(xt[:nv]), ptrs(on[:nv]), ptrs(ot[:nv]), None,
                             nj, blocks, reps, C.byref(ms))
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    inst = LpInstance(a.n, seed=0)
    m, n = inst.m, inst.n
    by = 4.0 * m * n
    say("batch_rate: benchmark_lp shape m = %d, n = %d, A = %.3f GB f32; 8 TB/s on 4 m n bytes = %.4f ms per pass" % (m, n, by / 1e9, by / PEAK * 1e3))
    rng = np.random.default_rng(0)
    D = T.DeviceBuffer
    xn = [D.from_host(rng.standard_normal(n).astype(np.float32)) for _ in range(8)]
    xt = [D.from_host(rng.standard_normal(m).astype(np.float32)) for _ in range(8)]
    on, ot = [D(m) for _ in range(8)], [D(n) for _ in range(8)]

    # ---- 1. one launch: NV pairs against the single-vector kernel (the yardstick), every tiling, rounds interleaved ----
    say()
    say("1. ms per launch (HIP events, best of %d launches per round, %d rounds interleaved; min / median over rounds)" % (a.reps, a.rounds))
    cfgs = [(1, 0, 0)] + [(nv, nj, bl) for nv in (2, 4, 8) for nj in ((1, 2) if nv < 8 else (1,)) for bl in (0, 2048, 4096, 8192)]
    res = {c: [] for c in cfgs}
    for c in cfgs:                                   # warm-up of every shape
        kernel_ms(inst, c[0], c[1], c[2], xn, xt, on, ot, 3)
    for _ in range(a.rounds):
        for c in cfgs:
            res[c].append(kernel_ms(inst, c[0], c[1], c[2], xn, xt, on, ot, a.reps))
    base = min(res[(1, 0, 0)])
    say("   %-34s %9s %9s %8s %10s %12s" % ("kernel / tiling", "min ms", "median", "of 8TB/s", "x single", "ms per pair"))
    best = {}
    for c in cfgs:
        lo, med = min(res[c]), float(np.median(res[c]))
        name = "dual_gemv_k (NV = 1, default plan)" if c[0] == 1 else "NV = %d  nj = %d  grid %s" % (c[0], c[1], c[2] or "default")
        say("   %-34s %9.4f %9.4f %8.3f %10.3f %12.4f" % (name, lo, med, by / PEAK * 1e3 / lo, lo / base, lo / c[0]))
        if c[0] not in best or lo < best[c[0]][0]:
            best[c[0]] = (lo, c)
    for nv in (2, 4, 8):
        say("   best NV = %d: %.4f ms = %.2fx the single-vector launch for %d pairs (%.2fx the work per ms)"
            % (nv, best[nv][0], best[nv][0] / base, nv, nv * base / best[nv][0]))
    say("   NV = 8 once %.4f ms  vs  NV = 4 twice %.4f ms" % (best[8][0], 2 * best[4][0]))
    for b in xn + xt + on + ot:
        b.free()

    # ---- 2. the loop: instance-iterations per second, batch against one carried solver, same matrix, same process ----
    say()
    say("2. instance-iterations per second (host clock around run() of %d iterations, which ends in a synchronise; autotune on;" % a.steps)
    say("   best / median of %d interleaved rounds); fraction of 8 TB/s = (2 passes x 4 m n bytes x instance-iterations / s) / 8 TB/s" % a.rounds)
    p = T.SolverParam()
    p.eps_acc, p.eps_inf, p.max_iter = 1e-30, 1e-30, None
    bs, cs = [], []
    for i in range(8):
        h = _gen(m, i, STREAM_H, 0, 0)
        h[:n] = 0.0
        bs.append(D.from_host(h))
        cs.append(D.from_host(-_gen(n, i, STREAM_C, 0, 0)))
    runs = {}
    fs = T.FusedSolver(n, m, inst.mat_a, bs[0], cs[0], inst.seg_type, inst.seg_len, p, "carried")
    runs["FusedSolver carried (1 instance)"] = (fs, 1)
    for B, g in ((1, 8), (2, 8), (4, 8), (8, 8), (8, 4)):
        bt = T.BatchSolver(n, m, inst.mat_a, bs[:B], cs[:B], inst.seg_type, inst.seg_len, p, max_group=g)
        runs["BatchSolver B = %d%s" % (B, "" if g == 8 else " as two groups of 4")] = (bt, B)
    times = {k: [] for k in runs}
    for k, (s, B) in runs.items():
        s.run(30, poll_every=30)                     # warm-up
    for _ in range(a.rounds):
        for k, (s, B) in runs.items():
            lib.thip_sync()
            t0 = time.perf_counter()
            s.run(a.steps, poll_every=a.steps)
            times[k].append(time.perf_counter() - t0)
    single = None
    say("   %-44s %10s %10s %12s %12s %9s %9s" % ("", "ms / iter", "median", "inst-it / s", "x single", "of 8TB/s", "passes"))
    for k, (s, B) in runs.items():
        lo, med = min(times[k]) / a.steps, float(np.median(times[k])) / a.steps
        rate = B / lo
        if single is None:
            single = rate
        passes = s.passes()[0] if B == 1 and not hasattr(s, "n_inst") else s.info()["passes_per_iteration"]
        say("   %-44s %10.4f %10.4f %12.1f %12.3f %9.3f %9d" % (k, lo * 1e3, med * 1e3, rate, rate / single, 2 * by * rate / PEAK, passes))
        if hasattr(s, "n_inst"):
            pl = s.info()["plans"]
            say("       plans: " + ", ".join("NV=%d nj=%d grid=%d %.3f ms" % (nv, v["rows_groups_per_lane"], v["target_workgroups"], v["autotune_ms"])
                                           for nv, v in pl.items() if v["target_workgroups"]))
    r4 = 4 / (min(times["BatchSolver B = 4"]) / a.steps)
    say()
    say("B = 4 condition: %.1f instance-iterations / s against %.1f of the single carried solver: %s" % (r4, single, "HOLDS" if r4 > single else "FAILS"))
    for s, _ in runs.values():
        s.destroy()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if r4 > single else 1


if __name__ == "__main__":
    sys.exit(main())
