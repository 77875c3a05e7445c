"""CPU-only: oracle.wcx_oracle.normalize_repeat_vec (the vectorised restatement the normalise-path GPU
tests compare with) against the loop oracle normalize_repeat on the planted references and samples
of tests/normalize_cases.py, and the case table of those tests against the dispatch rule."""
import warnings

import numpy as np
import pytest

import normalize_cases as NC
from oracle import wcx_oracle as O


def _check(got, want, what):
    for nm, a, b in zip(("z", "r", "n", "m_lr", "m_z"), got, want):
        a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
        assert np.array_equal(np.isnan(a), np.isnan(b)), what + ": nan " + nm
        assert np.array_equal(np.isposinf(a), np.isposinf(b)), what + ": +inf " + nm
        assert np.array_equal(np.isneginf(a), np.isneginf(b)), what + ": -inf " + nm
        if nm == "n":
            assert np.array_equal(a, b), what + ": n"
        else:
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=what + ": " + nm)


@pytest.mark.parametrize("k,lay,cut", [(1, "A", NC.CUT), (63, "Gb", NC.CUT), (65, "A", NC.WIDE),
                                       (129, "Gs", NC.CUT), (200, "Gb", NC.WIDE), (513, "A", NC.CUT)])
def test_vectorised_oracle_equals_loop_oracle(k, lay, cut):
    ref, info = NC.make_reference(k, lay, 5 + k)
    xs = NC.make_samples(info, 9, 6 + k, dead=1)
    ct, cp = NC.case_ct(info, lay)
    args = (ref["masked_bins_per_chr"], ref["masked_bins_per_chr_cum"], ref["indexes"],
            ref["distances"], cut, ct, cp)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for s in (0, 1, 2, 7, 8):
            want = O.normalize_repeat(xs[s], *args)
            got = O.normalize_repeat_vec(xs[s], *args)
            _check(got, want, "k=%d %s sample %d" % (k, lay, s))
            if s == 0:    # the planted edges are in the data: +inf z of all-zero sets, padding wrap
                assert np.isposinf(want[0]).any() or k < 33
                assert np.isnan(want[0]).any()
            if s == 1:
                assert np.all(want[2] == 0) and np.isnan(want[3]) and np.isnan(want[4])


def test_case_table_reaches_every_path():
    """Each row of the dispatch table (tests/normalize_cases.py: norm_path) is reached with at least
    two refsizes; every values-per-lane width reaches every kernel that is templated on it; the
    tile / lane-tile boundaries of the sample count and the three gonosome layouts are all present."""
    by_path = {}
    for k, ns, lay, cut in NC.CASES:
        B = int(NC.layout(k, lay).sum())
        ct = int(NC.layout(k, lay)[:22].sum()) if lay != "A" else 0
        by_path.setdefault(NC.norm_path(k, ns, B, ct), []).append((k, ns, lay, cut))
    assert set(by_path) == {"single", "tile", "rank", "gtile", "wide", "rows"}
    for p, cs in by_path.items():
        assert len({c[0] for c in cs}) >= 2, p
    ipls = {p: {NC.ipl_for(c[0]) for c in cs} for p, cs in by_path.items()}
    every = set(range(1, 9))
    assert ipls["rank"] >= every                                      # k_norm_median_rank<IPL>
    assert ipls["tile"] | ipls["gtile"] | ipls["wide"] >= every       # k_normalize_pass_tile<IPL, 8>
    assert ipls["rank"] | ipls["gtile"] | ipls["wide"] >= every       # lanes / incr (ipl argument)
    assert ipls["single"] | ipls["rows"] >= every | {16, 32}          # k_normalize_pass<IPL>
    assert ipls["rows"] >= {16, 32} and ipls["single"] >= {16, 32}
    ks = {c[0] for c in NC.CASES}
    assert ks >= {1, 63, 64, 65, 128, 129, 200, 256, 320, 384, 448, 511, 512, 513, 1024, 1025, 2048}
    assert {c[1] for c in NC.CASES} >= {1, 2, 8, 9, 15, 16, 17, 64, 65, 128, 129}
    assert {c[2] for c in by_path["rank"]} >= {"A", "Gb"}            # ct = 0 and ct > 0 on the rank path
    assert {c[2] for c in NC.CASES} == {"A", "Gs", "Gb"}
    assert {c[3] for c in NC.CASES} == {NC.CUT, NC.WIDE}
