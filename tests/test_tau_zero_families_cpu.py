"""The inputs of tests/test_gpu_tau_zero.py, validated with the CPU oracle alone (no GPU): every family of
tests/tau_zero_problems.py has the shape the kernels need, reaches the verdict it is built for within MAX_VERDICT_ITER iterations,
sends tau to zero inside the first 100 iterations -- F3 and F4 with tau coming back above eps_zero before it dies for good -- and
the snap selection leaves enough DECISIVE iterations of either kind, so that the GPU tests cannot go vacuous.

Decisive: the value of tau before the clamp max(., 0),
    pre_i = tau_{i-1} + t_tau (-(c.u_{i-1}) - (b.v_{i-1})),
is at least 10 tol(i) (max|x_i| + max|y_i|) away from zero.  An f32 iterate within tol of the oracle's moves pre by at most
tol (max|x| + max|y|), because t_tau (|c|_1 + |b|_1) <= 1; so at a decisive iteration the f32 loop and the f64 oracle are on the
same side of eps_zero, and kind, criteria and tau == 0 can be compared."""
import numpy as np
import pytest

import tau_zero_problems as Z

NAMES = ["F1", "F2", "F3", "F4", "F5", "F6-ok", "F6-infeasible", "F6-unbounded"]
FLIP_BACK = ("F3", "F4")


def _get(name):
    if name.startswith("F6"):
        q = ["F6-ok", "F6-infeasible", "F6-unbounded"].index(name)
        return Z.family("F6")[q], Z.plan("F6")[q]
    return Z.family(name), Z.plan(name)


@pytest.mark.parametrize("name", NAMES)
def test_family_shape(name):
    fam, _ = _get(name)
    assert fam.name == name and fam.m % 4 == 0 and fam.n >= 64
    A = fam.A
    assert A.dtype == np.float32 and fam.vec_b.dtype == np.float32 and fam.vec_c.dtype == np.float32
    assert np.array_equal(fam.mat_a.reshape((fam.n, fam.m)).T, A)
    # no two rows and no two columns are equal, and A is not symmetric where it is square
    assert len({r.tobytes() for r in A}) == fam.m and len({c.tobytes() for c in A.T}) == fam.n
    assert fam.m != fam.n or not np.array_equal(A, A.T)
    want = {"F1": (128, 64), "F2": (64, 64), "F3": (256, 96), "F4": (160, 200), "F5": (588, 64)}.get(name, (64, 64))
    assert (fam.m, fam.n) == want


def test_f3_cones_are_short_and_f4_has_a_long_one():
    f3, f4 = Z.family("F3"), Z.family("F4")
    assert set(f3.seg_type) == {Z.CONE_SOC} and max(f3.seg_len) <= 129          # all_soc_short: the m-tail is sw_cone_k
    assert max(l for t, l in zip(f4.seg_type, f4.seg_len) if t == Z.CONE_SOC) > 129     # the three-launch m-tail
    f5 = Z.family("F5")
    assert [l for t, l in zip(f5.seg_type, f5.seg_len) if t == Z.CONE_PSD] == [6 * 7 // 2, 33 * 34 // 2]


def test_f6_shares_f2s_matrix():
    f2, f6 = Z.family("F2"), Z.family("F6")
    for f in f6:
        assert np.array_equal(f.A, f2.A) and f.seg_type == f2.seg_type and f.seg_len == f2.seg_len
    assert np.array_equal(f6[2].vec_b, f2.vec_b) and np.array_equal(f6[2].vec_c, f2.vec_c)
    assert np.array_equal(f6[0].vec_b, f6[2].vec_b) and np.array_equal(f6[0].vec_c, f6[1].vec_c)
    assert not np.array_equal(f6[0].vec_b, f6[1].vec_b) and not np.array_equal(f6[0].vec_c, f6[2].vec_c)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_verdict_within_the_bound(name):
    fam, pl = _get(name)
    print("tau_zero family %-13s verdict %d at iteration %d, kind flips at %s" % (name, pl.status, pl.iters, pl.flips))
    assert pl.status == fam.verdict, (name, pl.status)
    assert pl.iters <= Z.MAX_VERDICT_ITER, (name, pl.iters)


@pytest.mark.parametrize("name", NAMES)
def test_clamp_formula_reproduces_the_oracles_tau(name):
    fam, pl = _get(name)
    # two f64 dot products of n + m terms in different orders, scaled by t_tau <= 1 / (|c|_1 + |b|_1)
    bound = 2 * (fam.n + fam.m + 2) * 2.0 ** -53 * max(1.0, np.abs(pl.snaps[:, pl.N:]).max())
    err = np.abs(np.maximum(pl.pre, 0.0) - pl.tau).max()
    print("tau_zero family %-13s max |max(pre, 0) - tau| = %.2e (bound %.2e)" % (name, err, bound))
    assert err <= bound, (name, err, bound)
    assert [int(t > 1e-12) for t in pl.tau] == [1 - k for k in pl.kinds]
    assert pl.precond[pl.N - 1] * (np.abs(fam.vec_c).sum(dtype=np.float64) + np.abs(fam.vec_b).sum(dtype=np.float64)) <= 1.0 + 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_snap_selection_is_not_vacuous(name):
    fam, pl = _get(name)
    assert set(Z.BASE_SNAPS) <= set(pl.chosen) and all(0 <= i < Z.N_SNAP for i in pl.chosen)
    for f in pl.flips:
        assert f - 1 in pl.chosen and f in pl.chosen and pl.kinds[f] != pl.kinds[f - 1]
    before, ones, after = Z.counts(pl)
    print("tau_zero family %-13s chosen %s decisive %s: %d of kind 0 before the first zero, %d of kind 1, %d of kind 0 after"
          % (name, pl.chosen, [i for i in pl.chosen if pl.decisive[i]], before, ones, after))
    if name == "F6-ok":
        assert pl.kinds == [0] * Z.N_SNAP and before == len(pl.chosen)        # the bounded slot never leaves tau > 0
        return
    assert before >= 1 and ones >= 3, (name, before, ones)
    if name in FLIP_BACK:
        first1 = pl.kinds.index(1)
        assert 0 in pl.kinds[first1:], name                                   # tau returns above eps_zero before iteration 100
        assert after >= 1, (name, after)
        assert fam.flips_back
