"""Problem-iterations per second of the SDP batch (totsu_amd.SdpBatchSolver: the mid batch's iteration with the PSD cones projected on
chip by the problem's workgroup) on the five layouts the family exists for --

    45 x 6       random_sdp(6, 9): one cone of order 9
    300 x 6      random_sdp(6, 24): order 24
    588 x 64     family F5 of tests/tau_zero_problems.py: orders 6 and 33 and 6 nonnegative rows
    560 x 528    partitioning_sdp(4, 8): order 32 and 32 zero-cone rows
    1176 x 48    random_sdp(48, 48): order 48

-- at P = 16, 64, 256 and 1024 problems, eps_acc = eps_inf = 1e-30 so that nothing stops, in one process on one device, against

    the baseline: one FusedSolver(schedule="carried") per problem, one after the other (sixteen problems: its rate does not depend
    on P) -- the only route for such problems before this family;
    the same A traffic with no projection: MidBatchSolver on the same m x n, the same A, b, c, every row in ONE nonnegative segment.
    What an SDP batch iteration takes beyond that is the projection: its share of the iteration is 1 - rate_sdp / rate_mid.

Host clock around run() with the stream synchronised; construction, init and a warm-up run are outside the timed span; a window
lasts about --window seconds (the iteration count is scaled from a first short window), the median of three is reported with the
spread (tools/midbatch_rate.py, whose helpers these are).  No ratio is a condition: the figures are what they are.
profiles/sdpbatch_rate.txt.
    python tools/sdpbatch_rate.py [--window 0.3] [--base-iters 256] [--poll 32] [--sizes 16,64,256,1024] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from midbatch_rate import DISTINCT, F, T, _lib, compute_units, stacked, timed  # noqa: E402  (puts the package and tests/ on the path)
import tau_zero_problems as Z  # noqa: E402
from problems import partitioning_sdp, random_sdp  # noqa: E402


def tri(k):
    return k * (k + 1) // 2


def svec_scale(k):
    """per packed entry (upper triangle by columns): 1 on the diagonal, sqrt 2 off it -- what ProbSDP.dense() multiplies by"""
    jj = np.repeat(np.arange(k), np.arange(1, k + 1))
    ii = np.arange(tri(k)) - jj * (jj + 1) // 2
    return np.where(ii == jj, 1.0, np.sqrt(2.0))


def family(name, mats, seg_type, seg_len):
    """mats: (A (m x n), b, c) per problem"""
    m, n = mats[0][0].shape
    return dict(name="%s %d x %d" % (name, m, n), n=n, m=m, a=np.stack([np.asfortranarray(A.astype(F)).ravel(order="F") for A, _, _ in mats]),
                b=np.stack([b.astype(F) for _, b, _ in mats]), c=np.stack([c.astype(F) for _, _, c in mats]),
                seg_type=list(seg_type), seg_len=list(seg_len))


def sdp_family(n, k):
    sc = svec_scale(k)
    mats = []
    for s in range(DISTINCT):
        c, syms = random_sdp(n, k, seed=s)
        mats.append((np.stack([sy * sc for sy in syms[:-1]], axis=1), -(syms[-1] * sc), c))
    return family("SDP order %d" % k, mats, [_lib.CONE_PSD], [tri(k)])


def f5_family():
    fams = [Z.f5(seed=5 + s) for s in range(DISTINCT)]
    return family("F5 orders 6, 33", [(f.A, f.vec_b, f.vec_c) for f in fams], fams[0].seg_type, fams[0].seg_len)


def partitioning_family(grid):
    l = grid[0] * grid[1]
    sc = svec_scale(l)
    mats = []
    for s in range(DISTINCT):
        w, syms_f, mat_a, vec_b = partitioning_sdp(*grid, seed=s)
        A = np.vstack([np.array(syms_f[:-1]).T * sc[:, None], mat_a])
        mats.append((A, np.concatenate([-(syms_f[-1] * sc), vec_b]), w))
    return family("partitioning %d x %d, order %d" % (grid + (l,)), mats, [_lib.CONE_PSD, _lib.CONE_ZERO], [tri(l), l])


def batch_rate(cls, fam, seg, P, p, a):
    """(problem-iterations per second: median, low, high; info) of one own-A batch class at P problems"""
    bufs = [stacked(fam[k], P) for k in ("a", "b", "c")]
    sb = cls(fam["n"], fam["m"], bufs[0], bufs[1], bufs[2], seg[0], seg[1], p)
    sb.run(8, a.poll)                                  # warm-up
    probe = 2 * a.poll
    iters = max(probe, int(probe * a.window / timed(lambda: sb.run(probe, a.poll))) // a.poll * a.poll)
    dts = sorted(timed(lambda: sb.run(iters, a.poll)) for _ in range(3))
    res = [sb.status(i) for i in (0, P - 1)]
    assert all(r.iters == 8 + probe + 3 * iters and r.state == _lib.ST_RUNNING for r in res), [(r.iters, r.state) for r in res]
    info = sb.info()
    sb.destroy()
    for d in bufs:
        d.free()
    return P * iters / dts[1], P * iters / dts[2], P * iters / dts[0], info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--base-iters", type=int, default=256)
    ap.add_argument("--poll", type=int, default=32)
    ap.add_argument("--sizes", default="16,64,256,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init()
    cus = compute_units()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    p = T.SolverParam()
    p.eps_acc = p.eps_inf = 1e-30
    say("sdpbatch_rate: problem-iterations per second, eps_acc = eps_inf = 1e-30 (nothing stops), poll_every = %d, %d CUs" % (a.poll, cus))
    say("   sdp: SdpBatchSolver (cones one after another, x_y then x_s, waves 0 .. 3); mid: MidBatchSolver on the same A, b, c with every row")
    say("   nonnegative (the same A traffic, no projection); windows of about %.2f s, median of 3 (low .. high)" % a.window)
    say("   baseline: 16 x FusedSolver(\"carried\") in turn, %d iterations each, median of 3; projection share = 1 - sdp / mid" % a.base_iters)
    fams = [lambda: sdp_family(6, 9), lambda: sdp_family(6, 24), f5_family, lambda: partitioning_family((4, 8)), lambda: sdp_family(48, 48)]
    summary, lost = [], []
    for make in fams:
        fam = make()
        n, m = fam["n"], fam["m"]
        seg = (fam["seg_type"], fam["seg_len"])
        solvers = [T.FusedSolver(n, m, fam["a"][i], fam["b"][i], fam["c"][i], seg[0], seg[1], p, "carried") for i in range(16)]
        for fs in solvers:
            fs.run(8, a.poll)                          # warm-up
        dts = sorted(timed(lambda: [fs.run(a.base_iters, a.poll) for fs in solvers]) for _ in range(3))
        assert all(fs.status().iters == 8 + 3 * a.base_iters for fs in solvers)
        for fs in solvers:
            fs.destroy()
        base = 16 * a.base_iters / dts[1]
        say()
        say("%s  (segments %s of lengths %s; %.2f MB of A read per problem-iteration)" % (fam["name"], seg[0], seg[1], 8 * m * n / 1e6))
        say("   baseline  16 solvers in turn   %8.3f s (%.3f .. %.3f)  %10.0f problem-iterations/s  (%.1f us per iteration)"
            % (dts[1], dts[0], dts[2], base, 1e6 / base))
        for P in [int(v) for v in a.sizes.split(",")]:
            sdp, slo, shi, info = batch_rate(T.SdpBatchSolver, fam, seg, P, p, a)
            mid, mlo, mhi, _ = batch_rate(T.MidBatchSolver, fam, ([_lib.CONE_RPOS], [m]), P, p, a)
            share = 1.0 - sdp / mid
            say("   P = %-5d %4d threads %6d B LDS (%5d for the projection)  sdp %10.0f (%.0f .. %.0f)  mid %10.0f (%.0f .. %.0f) "
                "problem-iterations/s  ratio to baseline %7.2f  projection %4.1f %% of the iteration, (1 / sdp - 1 / mid) x min(P, CUs) = %6.1f us"
                % (P, info["threads"], info["lds_bytes"], info["psd_lds_bytes"], sdp, slo, shi, mid, mlo, mhi, sdp / base, 100.0 * share,
                   1e6 * min(P, cus) * (1.0 / sdp - 1.0 / mid)))
            summary.append((fam["name"], P, sdp / base, share))
            if sdp < base:
                lost.append((fam["name"], P))
    say()
    say("ratios to the baseline (projection share): " + "; ".join("%s P=%d %.2f (%.0f %%)" % (s[0], s[1], s[2], 100 * s[3]) for s in summary))
    say("the baseline wins at: %s" % ("; ".join("%s P=%d" % l_ for l_ in lost) if lost else "no shape and no P that was run"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
