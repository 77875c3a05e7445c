"""Every kernel path of the predict normalisation (wcx_predict_normalize_dev) against the NumPy oracle:
one sample, the tiled batch kernel, the lane-per-sample mask passes with the rank-median last pass or
the tiled last pass, the gonosomal pass (ct > 0), more than 128 samples, and refsizes 513..2048 --
each values-per-lane width (IPL 1..8, 16, 32) with a full and a partial last word.  The references
are synthetic (tests/normalize_cases.py) with planted edge rows (0, 1, 2, 32, 33 and all k selected
reference bins, all-zero reference sets of more than 32 bins, padding under a cut-off above 1e10)
and planted samples at lane-tile positions (heavy tails, NaN, negative values, integer values,
zero stretches, a sample with every row at n = 0).  Every sample of every case is compared: n
exactly, r / z to 1e-9, non-finite values (sign included) exactly."""
import warnings

import numpy as np
import pytest

import normalize_cases as NC
from oracle import wcx_oracle as O

pytestmark = pytest.mark.gpu

RTOL = 1e-9


@pytest.fixture(scope="module")
def pt():
    from wisecondorx_amd import predict_tools
    return predict_tools


def same_nonfinite(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
            and np.array_equal(np.isneginf(a), np.isneginf(b)))


def assert_sample(got, want, what):
    z, r, n, mlr, mz = got
    oz, orr, on, omlr, omz = want
    bad = np.flatnonzero(n != on)
    assert bad.size == 0, "%s: n differs at rows %s (%s vs %s)" % (what, bad[:8], n[bad[:8]], on[bad[:8]])
    for nm, a, b in (("z", z, oz), ("r", r, orr), ("m_lr/m_z", [mlr, mz], [omlr, omz])):
        if not same_nonfinite(a, b):
            a, b = np.asarray(a), np.asarray(b)
            d = np.flatnonzero((np.isnan(a) != np.isnan(b)) | (np.isposinf(a) != np.isposinf(b))
                               | (np.isneginf(a) != np.isneginf(b)))
            raise AssertionError("%s: non-finite %s differ at %s: kernel %s, oracle %s"
                                 % (what, nm, d[:8], a[d[:8]], b[d[:8]]))
    np.testing.assert_allclose(r, orr, rtol=RTOL, equal_nan=True, err_msg=what + ": r")
    np.testing.assert_allclose(z, oz, rtol=RTOL, atol=RTOL, equal_nan=True, err_msg=what + ": z")
    np.testing.assert_allclose([mlr, mz], [omlr, omz], rtol=RTOL, atol=1e-12, equal_nan=True,
                               err_msg=what + ": m_lr / m_z")


def run_case(pt, case, seed, dead):
    k, ns, lay, cut = case
    ref, info = NC.make_reference(k, lay, seed)
    xs = NC.make_samples(info, ns, seed + 1, dead=dead)
    ct, cp = NC.case_ct(info, lay)
    mb, cum = ref["masked_bins_per_chr"], ref["masked_bins_per_chr_cum"]
    idx, dist = ref["indexes"], ref["distances"]
    cache = {}            # _dev caches the device reference by suffix only: one dict per reference
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        np.testing.assert_allclose(pt.get_optimal_cutoff(ref, 5, cache), O.get_optimal_cutoff(dist, 5),
                                   rtol=1e-12)
        np.testing.assert_allclose(pt.get_weights(ref, "", cache), O.get_weights(dist), rtol=1e-12)
        z, r, n, mlr, mz = pt.normalize_repeat_batch(xs, ref, cut, ct, cp, "", cache)
        assert z.shape == (ns, info["B"] - ct)
        for s in range(ns):
            want = O.normalize_repeat_vec(xs[s], mb, cum, idx, dist, cut, ct, cp)
            assert_sample((z[s], r[s], n[s], mlr[s], mz[s]), want, "%s sample %d" % (NC.case_id(case), s))
        # the loop oracle itself on the first (planted) sample
        want = O.normalize_repeat(xs[0], mb, cum, idx, dist, cut, ct, cp)
        assert_sample((z[0], r[0], n[0], mlr[0], mz[0]), want, "%s sample 0 (loop oracle)" % NC.case_id(case))
    return xs, z, r, n, info, ct


@pytest.mark.parametrize("case", NC.CASES, ids=[NC.case_id(c) for c in NC.CASES])
def test_normalize_path_vs_oracle(pt, case):
    k, ns, lay, cut = case
    dead = 1 if ns >= 3 else None
    xs, z, r, n, info, ct = run_case(pt, case, 1000 + 7 * k + ns, dead)
    rows = info["rows"]
    # the planted edges reached the kernels: all-zero reference sets of > 32 bins give +inf for an
    # own value > 0, the dead sample has no reference bin anywhere
    zr = [i - ct for i in rows["zero_ref"] if i >= ct]
    if zr:
        own = xs[:, ct:][:, zr]
        pos = (own > 0) & (n[:, zr] > 32)
        assert pos.any() and np.all(np.isposinf(z[:, zr][pos]))
    if dead is not None:
        assert np.all(n[dead] == 0) and np.all(np.isnan(z[dead]))


def test_normalize_single_sample_all_rows_empty(pt):
    """One sample with every row at n = 0: m_z and m_lr through the one-sample nanmedian are NaN."""
    xs, z, r, n, info, ct = run_case(pt, NC.DEAD_SINGLE, 77, 0)
    assert np.all(n == 0)
