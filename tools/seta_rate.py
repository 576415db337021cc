"""What a round of "new values of A for every problem, pattern, b and c kept" costs on an own-A batch, two ways, measured in one process
with no figure promised in advance.  The workloads of tools/setbc_rate.py -- MidBatchSolver, benchmark_lp 256 x 128 per problem, and
SparseBatchSolver on partitioning_sdp(4, 8) (560 x 528, 560 entries) -- at P = 256, eight rounds with every stored entry of A
perturbed by 1 % per round, eps_acc = 1e-3.  Every route twice:
    (i)   replace(i, A_i, b_i, c_i, start=raw_iterate(i)) on every slot, run, solution(i) in a loop      (the route there was)
    (ii)  set_a(A, keep_iterate=True), run, solutions()                                                   (the iterate kept)
Per route: wall time per round (the host clock around data update, run and read-out), problem-iterations to stop, and the three
parts of the wall time.  Then one set_a over all P beside one set_bc over all P, best of 5.  The dense update moves 32 MB from
pageable host memory per round; the sparse one 4 bytes per entry.
The iteration counts of (i) and (ii) may differ slightly: a stopped problem's raw_iterate is x_x / tau * tau, one rounding from the
iterate that lies in the arena, which is what (ii) keeps.
profiles/seta_rate.txt.
    python tools/seta_rate.py [--prob 256] [--rounds 8] [--eps 1e-3] [--max-iter 200000] [--out FILE]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sdpbatch_rate import partitioning_family  # noqa: E402  (puts the package and tests/ on the path)
from warm_start_rate import F, T, _lib, benchmark_lp, lib  # noqa: E402
from totsu_amd.sparsebatch import csc_of_dense  # noqa: E402

ROUTES = (("(i)  replace(start=raw) + solution(i)", "replace"), ("(ii) set_a(keep_iterate) + solutions()", "keep"))


def leg(say, a, make, refill, rounds, b0, c0, P):
    """make(): a batch on round 0; refill(sb, i, r, start): replace of slot i with round r's A; rounds[r]: what set_a takes"""
    say("   %-42s %9s %9s %18s   %9s %9s %9s   %s" % ("", "wall s", "s / round", "problem-iterations", "update s", "run s", "read s", "states"))
    last = None
    for rep in range(2):
        for label, route in ROUTES:
            sb = make()
            sb.run(-1, a.poll)
            sb.solutions()                                        # (the staging buffer is there before the clock starts)
            lib.thip_sync()
            total, states, parts = 0, set(), [0.0, 0.0, 0.0]
            t_all = time.perf_counter()
            for r in range(1, len(rounds)):
                t0 = time.perf_counter()
                if route == "replace":
                    for i in range(P):
                        refill(sb, i, r, sb.raw_iterate(i))
                else:
                    sb.set_a(rounds[r], keep_iterate=True)
                t1 = time.perf_counter()
                res = sb.run(-1, a.poll)
                t2 = time.perf_counter()
                sols = [sb.solution(i) for i in range(P)] if route == "replace" else sb.solutions()
                t3 = time.perf_counter()
                parts = [parts[0] + t1 - t0, parts[1] + t2 - t1, parts[2] + t3 - t2]
                total += sum(q.iters + 1 for q in res)
                states |= set(q.state for q in res)
            lib.thip_sync()
            dt = time.perf_counter() - t_all
            say("   %-42s %9.3f %9.4f %18d   %9.3f %9.3f %9.3f   %s" % ("%s, run %d" % (label, rep + 1), dt, dt / (len(rounds) - 1), total,
                                                                          parts[0], parts[1], parts[2], sorted(states)))
            x = np.stack([s[0] for s in sols])
            if route == "replace":
                last = x
            else:
                say("       last round against (i): max |x - x'| / max(1, |x|) = %.2e" % float(np.abs(x - last).max() / max(1.0, np.abs(last).max())))
            if rep == 1 and route == "keep":
                for what, fn in (("one set_a over all %d" % P, lambda: sb.set_a(rounds[-1])),
                                 ("one set_a(keep_iterate) over all %d" % P, lambda: sb.set_a(rounds[-1], keep_iterate=True)),
                                 ("one set_bc over all %d" % P, lambda: sb.set_bc(b0, c0)),
                                 ("one set_bc(keep_iterate) over all %d" % P, lambda: sb.set_bc(b0, c0, keep_iterate=True))):
                    best = 1e30
                    for _ in range(5):
                        lib.thip_sync()
                        t0 = time.perf_counter()
                        fn()
                        lib.thip_sync()
                        best = min(best, time.perf_counter() - t0)
                    say("   %-42s %9.1f us (best of 5; the host's packing and the copies included)" % (what, 1e6 * best))
            sb.destroy()


def main():
    ap = argparse.ArgumentParser()
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
    P = a.prob
    say("seta_rate: eps_acc = %g, max_iter = %d, poll_every = %d, P = %d, %d rounds; wall time by the host clock around the data update, the"
        % (a.eps, a.max_iter, a.poll, P, a.rounds))
    say("run and the read-out of every round (the first solve, from zero, is not counted)")

    def perturb(v0, seed):
        rng = np.random.default_rng(seed)
        rounds = [v0]
        for _ in range(a.rounds):
            rounds.append((rounds[-1] * (1 + 0.01 * rng.standard_normal(v0.shape))).astype(F))
        return rounds

    # ---- dense ---------------------------------------------------------------------------------------------------------------------
    lps = [benchmark_lp(128, 1000 + q) for q in range(P)]
    c0 = np.stack([cc for cc, _, _ in lps])
    b0 = np.stack([hh for _, _, hh in lps])
    rounds = perturb(np.stack([np.asfortranarray(g).ravel(order="F") for _, g, _ in lps]), 21)
    say()
    say("dense: MidBatchSolver, benchmark_lp 256 x 128 per problem, every entry of A perturbed by 1 %% per round (%.1f MB per round)"
        % (rounds[0].nbytes / 1e6))
    leg(say, a, lambda: T.MidBatchSolver(128, 256, rounds[0], b0, c0, [_lib.CONE_RPOS], [256], p),
        lambda sb, i, r, start: sb.replace(i, rounds[r][i], b0[i], c0[i], start=start), rounds, b0, c0, P)

    # ---- sparse: replace validates, packs and uploads the blob too ---------------------------------------------------------------------
    fam = partitioning_family((4, 8))
    n, m, D = fam["n"], fam["m"], fam["a"].shape[0]
    cscs = [csc_of_dense(fam["a"][q % D], n, m) for q in range(P)]
    nnz = int(cscs[0][0][-1])
    assert all(int(t[0][-1]) == nnz for t in cscs)
    c1 = np.stack([fam["c"][q % D] for q in range(P)])
    b1 = np.stack([fam["b"][q % D] for q in range(P)])
    rounds1 = perturb(np.stack([t[2] for t in cscs]), 22)
    say()
    say("sparse: SparseBatchSolver, %s, %d entries per problem, every entry perturbed by 1 %% per round (%.2f MB per round)"
        % (fam["name"], nnz, rounds1[0].nbytes / 1e6))
    leg(say, a, lambda: T.SparseBatchSolver(n, m, cscs, b1, c1, fam["seg_type"], fam["seg_len"], p),
        lambda sb, i, r, start: sb.replace(i, (cscs[i][0], cscs[i][1], rounds1[r][i]), b1[i], c1[i], start=start), rounds1, b1, c1, P)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
