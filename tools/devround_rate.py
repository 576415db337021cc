"""What a round costs when its data is PRODUCED ON THE DEVICE (by torch) and its answers are wanted there: the two legs of
tools/seta_rate.py and tools/setbc_rate.py -- MidBatchSolver, benchmark_lp 256 x 128 per problem, and SparseBatchSolver on
partitioning_sdp(4, 8) -- at P = 256, eight rounds in which every stored entry of A and every entry of b and c moves by 1 %,
eps_acc = 1e-3.  Every route twice, no figure promised in advance:
    (i)   the host route as such a caller lives it: tensor.cpu(), set_a(keep) + set_bc(keep), run, solutions(), results back up
    (ii)  set_a_dev(keep) + set_bc_dev(keep) on the tensors, run, solutions_dev()                          (one device-to-device copy of A)
    (iii) dense only: the batch built over the caller's buffer, the round written there, set_a_dev(None)   (no copy of A)
Per route: wall time (the host clock around update, run and read-out of every round), the three parts, problem-iterations.  Then the
dense update alone, best of 5: set_a_dev with the copy, the in-place form, their difference as the copy kernel's rate, beside a
plain hipMemcpyAsync device to device of the same bytes on the same stream.
profiles/devround_rate.txt.
    python tools/devround_rate.py [--prob 256] [--rounds 8] [--eps 1e-3] [--max-iter 200000] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sdpbatch_rate import partitioning_family  # noqa: E402  (puts the package and tests/ on the path)
from warm_start_rate import F, T, _lib, benchmark_lp, lib  # noqa: E402
from totsu_amd.sparsebatch import csc_of_dense  # noqa: E402

ROUTES = (("(i)   .cpu() + set_a/set_bc + solutions() + up", "host"), ("(ii)  set_a_dev + set_bc_dev + solutions_dev", "dev"),
          ("(iii) in place: set_a_dev(None) + set_bc_dev", "inplace"))


def rounds_on_device(v0, b0, c0, n_rounds, seed):
    """the rounds' data as torch tensors on the GPU, each 1 % multiplicative noise on the one before, made there"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    out = [tuple(torch.from_numpy(np.ascontiguousarray(v, F)).cuda() for v in (v0, b0, c0))]
    for _ in range(n_rounds):
        out.append(tuple((t * (1 + 0.01 * torch.randn(t.shape, generator=g, device="cuda", dtype=torch.float32))).contiguous() for t in out[-1]))
    torch.cuda.synchronize()
    return out


def leg(say, a, make, rounds, P, dense):
    """make(mats or None): a batch on round 0 -- over the given DeviceBuffer of A where one is handed in (dense)"""
    say("   %-50s %9s %9s %18s   %9s %9s %9s   %s" % ("", "wall s", "s / round", "problem-iterations", "update s", "run s", "read s", "states"))
    for rep in range(2):
        for label, route in ROUTES:
            if route == "inplace" and not dense:
                continue
            held = T.DeviceBuffer.from_host(rounds[0][0].cpu().numpy()) if route == "inplace" else None
            view = torch.as_tensor(held, device="cuda").view(rounds[0][0].shape) if held is not None else None
            sb = make(held)
            sb.run(-1, a.poll)
            sb.solutions()
            for d in sb.solutions_dev():                          # (the staging buffers are there before the clock starts)
                d.free()
            torch.cuda.synchronize()
            lib.thip_sync()
            total, states, parts = 0, set(), [0.0, 0.0, 0.0]
            t_all = time.perf_counter()
            for r in range(1, len(rounds)):
                va, vb, vc = rounds[r]
                t0 = time.perf_counter()
                if route == "host":
                    sb.set_a(va.cpu().numpy(), keep_iterate=True)
                    sb.set_bc(vb.cpu().numpy(), vc.cpu().numpy(), keep_iterate=True)
                elif route == "dev":
                    sb.set_a_dev(va, keep_iterate=True)
                    sb.set_bc_dev(vb, vc, keep_iterate=True)
                else:
                    view.copy_(va)                               # (the producer writes its round where the batch reads it)
                    torch.cuda.current_stream().synchronize()   # (no tensor is handed over, so the caller orders its own stream)
                    sb.set_a_dev(None, keep_iterate=True)
                    sb.set_bc_dev(vb, vc, keep_iterate=True)
                t1 = time.perf_counter()
                res = sb.run(-1, a.poll)
                t2 = time.perf_counter()
                if route == "host":
                    sols = sb.solutions()
                    x = torch.from_numpy(np.concatenate([s[0] for s in sols])).cuda()
                    y = torch.from_numpy(np.concatenate([s[1] for s in sols])).cuda()
                    torch.cuda.synchronize()
                else:
                    out = sb.solutions_dev()
                    x = torch.as_tensor(out[0], device="cuda").clone()
                    torch.cuda.synchronize()
                    for d in out:
                        d.free()
                t3 = time.perf_counter()
                parts = [parts[0] + t1 - t0, parts[1] + t2 - t1, parts[2] + t3 - t2]
                total += sum(q.iters + 1 for q in res)
                states |= set(q.state for q in res)
            lib.thip_sync()
            dt = time.perf_counter() - t_all
            say("   %-50s %9.3f %9.4f %18d   %9.3f %9.3f %9.3f   %s" % ("%s, run %d" % (label, rep + 1), dt, dt / (len(rounds) - 1), total,
                                                                          parts[0], parts[1], parts[2], sorted(states)))
            if rep == 1 and route == "inplace":
                copy_rate(say, sb, rounds[-1][0], view)
            sb.destroy()
            if held is not None:
                del view
                held.free()


def best_of(fn, reps=5):
    best = 1e30
    for _ in range(reps):
        lib.thip_sync()
        t0 = time.perf_counter()
        fn()
        lib.thip_sync()
        best = min(best, time.perf_counter() - t0)
    return best


def copy_rate(say, sb, va, view):
    """the dense update alone on a batch over the caller's buffer: with the copy, in place, and a plain runtime copy of the same bytes"""
    nbytes = va.numel() * 4
    with_copy = best_of(lambda: sb.set_a_dev(va, keep_iterate=True))
    in_place = best_of(lambda: sb.set_a_dev(None, keep_iterate=True))
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = C.c_void_p(_lib.load().thip_get_stream())
    plain = best_of(lambda: hip.hipMemcpyAsync(view.data_ptr(), va.data_ptr(), nbytes, 3, stream))
    say("   one set_a_dev(values, keep) over all: %9.1f us; set_a_dev(None, keep): %9.1f us (best of 5, tables and the status read included)"
        % (1e6 * with_copy, 1e6 * in_place))
    if with_copy > in_place:
        say("   the difference, check of the source and copy kernel on %.1f MB: %9.1f us = %.0f GB/s moved (read + written: twice that)"
            % (nbytes / 1e6, 1e6 * (with_copy - in_place), nbytes / (with_copy - in_place) / 1e9))
    say("   a plain hipMemcpyAsync device to device of the same bytes, launch to synchronisation: %9.1f us = %.0f GB/s moved"
        % (1e6 * plain, nbytes / plain / 1e9))


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
    say("devround_rate: eps_acc = %g, max_iter = %d, poll_every = %d, P = %d, %d rounds; the round's A, b and c are torch tensors on the GPU;"
        % (a.eps, a.max_iter, a.poll, P, a.rounds))
    say("wall time by the host clock around the data update, the run and the read-out of every round (the first solve is not counted)")

    lps = [benchmark_lp(128, 1000 + q) for q in range(P)]
    c0 = np.stack([cc for cc, _, _ in lps]).astype(F)
    b0 = np.stack([hh for _, _, hh in lps]).astype(F)
    a0 = np.stack([np.asfortranarray(g).ravel(order="F") for _, g, _ in lps]).astype(F)
    rounds = rounds_on_device(a0, b0, c0, a.rounds, 21)
    say()
    say("dense: MidBatchSolver, benchmark_lp 256 x 128 per problem (%.1f MB of A per round)" % (a0.nbytes / 1e6))
    leg(say, a, lambda held: T.MidBatchSolver(128, 256, a0 if held is None else held, b0, c0, [_lib.CONE_RPOS], [256], p), rounds, P, True)

    fam = partitioning_family((4, 8))
    n, m, D = fam["n"], fam["m"], fam["a"].shape[0]
    cscs = [csc_of_dense(fam["a"][q % D], n, m) for q in range(P)]
    nnz = int(cscs[0][0][-1])
    assert all(int(t[0][-1]) == nnz for t in cscs)
    c1 = np.stack([fam["c"][q % D] for q in range(P)]).astype(F)
    b1 = np.stack([fam["b"][q % D] for q in range(P)]).astype(F)
    rounds1 = rounds_on_device(np.stack([t[2] for t in cscs]).astype(F), b1, c1, a.rounds, 22)
    say()
    say("sparse: SparseBatchSolver, %s, %d entries per problem (%.2f MB of values per round)" % (fam["name"], nnz, 4e-6 * nnz * P))
    leg(say, a, lambda held: T.SparseBatchSolver(n, m, cscs, b1, c1, fam["seg_type"], fam["seg_len"], p), rounds1, P, False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
