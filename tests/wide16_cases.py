"""What the tests of the wide batch over a 16-bit A share (tests/test_gpu_wide16batch.py, tests/test_wide16batch_cpu.py): the helpers
of the wide suite that live in a test file there, restated (the arena as it lies on the device, the bitwise state, the shapes beyond
the old rules, the padded tau -> 0 families), and the twin -- a WideBatchSolver over the widened matrices W in f32 (tests/mid16_cases.py),
which a Wide16BatchSolver must equal bit for bit.  A plain module, like tests/ownbatch_cases.py and tests/mid16_cases.py."""
import ctypes as C

import numpy as np

import mid16_cases as M
import tau_zero_problems as Z
from ownbatch_cases import F, _D, _edge, _psd_block, _sdp_dense, _socp_dense, _View, tri

LDS = 163840
KINDS = M.KINDS


def rule(n, m, max_k=0):
    """the wide batch's LDS map (README.md, tests/test_widebatch_cpu.py)"""
    return 4 * (6208 + 3 * n + 3 * m) + ((m + 3) & ~3) + (49920 if max_k > 32 else 0)


def old_rule(n, m, max_k=0):
    """the mid / SDP batch's"""
    return 4 * (6208 + 8 * n + 13 * m) + ((m + 3) & ~3) + (49920 if max_k > 32 else 0)


def param(T, **kw):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def arena(T, sb):
    """the whole arena of a batch as it lies on the device, one row per problem"""
    from totsu_amd._lib import lib
    addr, size = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    lib.thip_test_ownbatch_addresses(sb.h, addr, size)
    assert addr[0] and size[0] == sb.info()["arena_bytes"]
    a = _View(T, type("B", (), {"ptr": addr[0]})(), 0, size[0] // 4).to_host()
    return a.reshape(sb.n_prob, -1)


def blocks(sb):
    return [(s.state, s.iters, s.kind, s.cri, s.tau, s.kappa, s.norm_b, s.norm_c) for s in sb.statuses()]


def state(T, sb, floats=None):
    """everything the contract covers, bit for bit: every arena block (`floats` of it from the front; None: all 6 n + 11 m), the
    status blocks, solutions() and every problem's preconditioner"""
    a = arena(T, sb)
    return (a if floats is None else a[:, :floats]).copy(), blocks(sb), sb.solutions(), [sb.precond(i) for i in range(sb.n_prob)]


def same_state(got, want, what, floats=None):
    ga, wa = (got[0], want[0]) if floats is None else (got[0][:, :floats], want[0][:, :floats])
    assert ga.shape == wa.shape and np.array_equal(ga.view(np.uint32), wa.view(np.uint32)), (what, "arena")
    assert repr(got[1]) == repr(want[1]), (what, got[1], want[1])
    for k in (2, 3):
        for (gx, gy), (wx, wy) in zip(got[k], want[k]):
            assert np.array_equal(gx.view(np.uint32), wx.view(np.uint32)) and np.array_equal(gy.view(np.uint32), wy.view(np.uint32)), (what, k)


def widened_problems(sb, ds):
    """the problems of ds with the matrices the 16-bit batch sb solves them with"""
    return [M.WDense(d, sb.widened(i)) for i, d in enumerate(ds)]


def pair(T, ds, kind, p=None, **kw):
    """(a Wide16BatchSolver over ds, its twin: a WideBatchSolver over the widened matrices on the same b, c and cones)"""
    sb = T.Wide16BatchSolver.from_dense(ds, p, a_dtype=kind, **kw)
    try:
        return sb, T.WideBatchSolver.from_dense(widened_problems(sb, ds), p, **kw)
    except Exception:
        sb.destroy()
        raise


def both(fn, *solvers):
    for s in solvers:
        fn(s)


# ---- the shapes beyond the mid and the SDP batch's rules (tests/test_gpu_widebatch.py::_wide_case, without the oracle runs) --------

def mixed64(T):
    """3 nonnegative rows, an order-64 and an order-5 PSD cone, a second-order cone of 9 rows and a rotated one of 5: n = 2"""
    from totsu_amd import _lib
    n, ds = 2, []
    for s in range(2):
        rng = np.random.default_rng(640 + s)
        blocks_, bs, st, sl = [rng.standard_normal((3, n)).astype(F)], [np.abs(rng.standard_normal(3)).astype(F) + 1.0], [_lib.CONE_RPOS], [3]
        c0 = np.zeros(n, F)
        for q, k in enumerate((64, 5)):
            rows, b, c = _psd_block(T, n, k, 70 + q + 10 * s)
            blocks_.append(rows)
            bs.append(b)
            st.append(_lib.CONE_PSD)
            sl.append(tri(k))
            c0 = c0 + c
        for t, rows in ((_lib.CONE_SOC, 9), (_lib.CONE_ROTSOC, 5)):
            blocks_.append((rng.standard_normal((rows, n)) / 4).astype(F))
            b = (rng.standard_normal(rows) / 4).astype(F)
            b[0] = 3.0
            if t == _lib.CONE_ROTSOC:
                b[1] = 3.0
            bs.append(b)
            st.append(t)
            sl.append(rows)
        ds.append(_D(np.vstack(blocks_), np.concatenate(bs), c0 / 2, st, sl))
    return ds


_WIDE = {}


def wide_case(T, name):
    """(problems, largest PSD order), computed once: lp<m>x<n> (two LPs over the nonnegative cone), socp2600, mixed64, sdp48n837"""
    if name in _WIDE:
        return _WIDE[name]
    max_k = 0
    if name.startswith("lp"):
        m, n = (int(v) for v in name[2:].split("x"))
        ds = [_edge(m, n, s) for s in range(2)]
    elif name == "socp2600":
        ds = [_socp_dense(T, 60, [5, 1, 0, 17, 1200, 1367, 3], s)[0] for s in range(2)]
        assert all((d.m, d.n) == (2600, 60) for d in ds)
    elif name == "mixed64":
        max_k, ds = 64, mixed64(T)
    else:
        assert name == "sdp48n837", name
        max_k, ds = 48, [_sdp_dense(T, 837, 48, s) for s in range(2)]
    _WIDE[name] = (ds, max_k)
    return _WIDE[name]


# ---- the tau -> 0 families beyond the mid batch's rule (tests/test_gpu_widebatch.py::_padded) ---------------------------------------

PAD_M = 2600                       # rows of every padded family: 13 m alone is 33 800 floats


def padded(fam):
    """the family with inert rows appended -- a zero cone of zero rows, b = 0 -- up to PAD_M rows: the same problem, beyond the mid
    batch's rule (and, for F5, the SDP batch's)"""
    extra = PAD_M - fam.m
    assert extra > 0 and old_rule(fam.n, PAD_M, 33 if fam.psd else 0) > LDS
    A = np.vstack([fam.A, np.zeros((extra, fam.n), F)])
    return Z.Family(fam.name + "/padded", fam.n, A, np.concatenate([fam.vec_b, np.zeros(extra, F)]), fam.vec_c,
                    fam.seg_type + [Z.CONE_ZERO], fam.seg_len + [extra], fam.verdict, fam.flips_back)
