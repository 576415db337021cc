"""What the set_bc / solutions tests share (tests/test_gpu_setbc.py, tests/test_setbc_cpu.py): the six own-A batch families with the
problem sets of the start-iterate tests (the smallest that reach every code path: 16-byte and 4-byte loads, both LDS maps of the PSD
cones, both thread classes of a ragged batch, a resident and a streamed blob), the new (b, c) -- 1 % multiplicative noise with a
fixed seed -- and the whole readable state of a problem for the bitwise comparisons.  A plain module, like tests/warm_cases.py."""
import copy

import numpy as np

from ownbatch_cases import F, _edge
from sparse_cases import csc_of, sparse_problem
from warm_cases import oracle_run, sdp_numpy, socp_numpy, sparse40x30

FAMILIES = ["small", "mid", "sdp", "ragged", "sparse", "raggedsparse"]
RAGGED = ("ragged", "raggedsparse")


def with_bc(d, b, c, rowabs="same"):
    e = copy.copy(d)
    e.vec_b, e.vec_c = np.asarray(b, F), np.asarray(c, F)
    if not isinstance(rowabs, str):
        e.vec_b_rowabs = None if rowabs is None else np.asarray(rowabs, F)
    return e


def perturbed(d, seed):
    """d with b and c under 1 % multiplicative noise (the construction of the start-iterate tests); its row sums, if any, stay"""
    rng = np.random.default_rng(77 + seed)
    return with_bc(d, d.vec_b * (1 + 0.01 * rng.standard_normal(d.m)), d.vec_c * (1 + 0.01 * rng.standard_normal(d.n)))


def rowsums(d, seed):
    """row sums that go with d's b and are not |b|: |b| + U(0.1, 1)"""
    rng = np.random.default_rng(505 + seed)
    return (np.abs(np.asarray(d.vec_b, F)) + rng.uniform(0.1, 1.0, d.m)).astype(F)


def param(T, arith=None, **kw):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    if arith:
        p.state_arith = arith
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Fam:
    """a family: its class, the workgroup sizes its test hook forces, its problem sets [(label, problems, SOCP pieces per problem or
    None, [extra keywords])], and how it is made and refilled"""

    def __init__(self, T, name):
        self.name = name
        self.cls = {"small": T.SmallBatchSolver, "mid": T.MidBatchSolver, "sdp": T.SdpBatchSolver, "ragged": T.RaggedBatchSolver,
                    "sparse": T.SparseBatchSolver, "raggedsparse": T.RaggedSparseBatchSolver}[name]
        self.forced = (64, 256, 1024) if name == "small" else (256, 1024)
        self.sparse = name in ("sparse", "raggedsparse")
        one = [{}]
        if name == "small":
            socp = [socp_numpy(s) for s in range(2)]
            self.sets = [("lp80x40", [_edge(80, 40, s) for s in range(3)], None, one), ("lp1x1", [_edge(1, 1, s) for s in range(2)], None, one),
                         ("socp102x12", [d for d, _ in socp], [p for _, p in socp], one)]
        elif name == "mid":
            self.sets = [("lp160x96", [_edge(160, 96, s) for s in range(2)], None, one),       # aligned: 16-byte loads
                         ("lp157x157", [_edge(157, 157, s) for s in range(2)], None, one)]     # m odd: the 4-byte path
        elif name == "sdp":
            self.sets = [("sdp45x6", [sdp_numpy(6, 9, s) for s in range(2)], None, one),
                         ("sdp561x6", [sdp_numpy(6, 33, 0)], None, one)]                        # order 33: the larger LDS map
        elif name == "ragged":                                                                  # both thread classes, 1 x 1 among them
            self.sets = [("five", [_edge(1, 1, 0), _edge(80, 40, 0), _edge(160, 96, 0), _edge(157, 157, 0), sdp_numpy(6, 9, 0)], None, one)]
        elif name == "sparse":
            self.sets = [("sp40x30", [sparse40x30(s) for s in range(3)], None, [{}, {"force_resident": 0}])]
        else:       # lp257x129 in a slot of m n entries cannot reside (streamed, the 1024-thread class); the others reside
            ds = [sparse40x30(0), sparse_problem("lp257x129", 0), sparse_problem("mixed145x40", 0), _edge(80, 40, 0)]
            self.sets = [("four", ds, None, [{"nnz_caps": [0, 257 * 129, 0, 3200]}])]

    def make(self, ds, p, forced=None, **kw):
        return self.cls.from_dense(ds, p, force_threads=forced, **kw)

    def replace(self, sb, i, d, start=None):
        sb.replace(i, csc_of(d) if self.sparse else d.mat_a, d.vec_b, d.vec_c, d.vec_b_rowabs, start=start)

    def set_bc(self, sb, ds, first=0, keep=False):
        sb.set_bc([d.vec_b for d in ds], [d.vec_c for d in ds], [d.vec_b_rowabs for d in ds], first=first, keep_iterate=keep)

    def oracle(self, label, q, d, pieces):
        return oracle_run("setbc/%s/%s/%d" % (self.name, label, q), d, socp=None if pieces is None else pieces[q])

    def cycled(self, label_index, P, kw):
        """the set's problems cycled to P, and the keywords that go with them"""
        _, ds, _, _ = self.sets[label_index]
        kw = dict(kw)
        if "nnz_caps" in kw:
            kw["nnz_caps"] = [kw["nnz_caps"][i % len(ds)] for i in range(P)]
        return [ds[i % len(ds)] for i in range(P)], kw


def full(sb, i):
    """everything of problem i that can be read: the preconditioner (with the two scalars), the raw iterate (with tau and kappa) and
    the status block (with the norms)"""
    st = sb.status(i)
    return sb.precond(i) + sb.iterate(i) + ((st.state, st.iters, st.kind, tuple(st.cri), st.tau, st.kappa, st.norm_b, st.norm_c),)


def same(g, w, tag=None):
    for k in range(4):
        assert np.array_equal(g[k], w[k]), (tag, k, np.abs(g[k] - w[k]).max())
    assert g[4] == w[4], (tag, g[4], w[4])
