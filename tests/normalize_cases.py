"""Synthetic references and sample batches for the normalise-path tests (test_gpu_normalize_paths.py,
test_oracle_normalize_vec.py): random indexes / distances over 24 chromosomes of uneven size, with
planted edge rows and planted samples; no search needed."""
import numpy as np

# 22 autosomes of uneven size (1570 bins at scale 1)
AUTO = [150, 130, 120, 110, 100, 95, 90, 85, 80, 75, 70, 65, 60, 55, 50, 45, 40, 38, 34, 30, 26, 22]
GONO = {"A": (40, 20), "Gs": (40, 20), "Gb": (330, 200)}   # chromosomes 23, 24 per layout
CUT = 0.25            # explicit cut-off: about 2/3 of a random row's gamma(4, 0.05) distances
WIDE = 2e10           # a cut-off above the padding distance: every entry selected, padding included
FAR = 1e12            # distance of the entries a planted row leaves out (above both cut-offs)
NSEL = (0, 1, 2, 32, 33)          # planted selection counts (plus "all k")
ZERO_N = (33, 40, 57, 64, 80)     # planted all-zero reference sets with more than 32 members
PLANT_AT = (0, 7, 8, 63, 64)      # lane-tile positions of the planted samples (plus the last one)


def ipl_for(k):
    """predict.hip: ipl_for -- values per lane of a reference row."""
    ipl = (k + 63) // 64
    return ipl if ipl <= 8 else (16 if ipl <= 16 else 32)


def norm_path(k, ns, B, ct):
    """The kernel path wcx_predict_normalize_dev takes (predict.hip, wcx_predict_normalize_dev:
    `tiled`, `lanes`, `rankmed`, with the default knobs):
      single -- one sample: k_normalize_pass, launch_nanmedian_wide;
      tile   -- 2..15 samples, k <= 512: k_normalize_pass_tile, k_nanmedian;
      rank   -- 16..128 samples, k <= 512, (B - ct) * 4 >= B: lanes + incr, last pass incr
                statistics + k_norm_median_rank;
      gtile  -- 16..128 samples, k <= 512, (B - ct) * 4 < B: lanes + incr, tiled last pass;
      wide   -- more than 128 samples, k <= 512: lanes + incr, tiled last pass;
      rows   -- 2 or more samples, k > 512: k_normalize_pass, one grid row per sample."""
    if ns == 1:
        return "single"
    if ipl_for(k) > 8:
        return "rows"
    if ns < 16:
        return "tile"
    if ns > 128:
        return "wide"
    return "rank" if (B - ct) * 4 >= B else "gtile"


def layout(k, lay):
    """masked_bins_per_chr of a case: autosomes scaled so that every chromosome's chr_data holds k
    distinct bins; gonosomes small (A, Gs) or a quarter of the bins and more (Gb)."""
    f = 1.0 if k <= 1100 else 1.5
    mb = [int(round(a * f)) for a in AUTO] + [int(round(g * f)) for g in GONO[lay]]
    return np.array(mb, dtype=np.int64)


def make_reference(k, lay, seed):
    """indexes / distances with planted rows.  Returns (ref dict, info dict)."""
    rng = np.random.default_rng(seed)
    mb = layout(k, lay)
    cum = np.cumsum(mb)
    B = int(cum[-1])
    start = cum - mb
    idx = np.empty((B, k), dtype=np.int32)
    for c in range(len(mb)):
        n_cd = B - int(mb[c])
        assert n_cd >= k
        for i in range(int(start[c]), int(cum[c])):
            idx[i] = rng.permutation(n_cd)[:k]
    dist = rng.gamma(4.0, 0.05, (B, k))

    def cd(row, c):          # chr_data index of bin `row` as seen from chromosome c
        return row if row < start[c] else row - mb[c]

    def chrom(row):
        return int(np.searchsorted(cum, row, side="right"))

    # two zero stretches (every sample is 0 there) referencing only each other: z = 0/0 = nan in
    # every pass, so they are never masked and stay all-zero reference sets for the rows below
    Z = np.arange(start[3] + 5, start[3] + 85)       # chromosome 4
    Z2 = np.arange(start[4] + 5, start[4] + 85)      # chromosome 5
    for a, b in ((Z, Z2), (Z2, Z)):
        for i in a:
            m = min(k, len(b))
            idx[i, :m] = [cd(j, chrom(i)) for j in b[:m]]
            dist[i, :m] = 0.01
            dist[i, m:] = FAR
    gstart = int(start[22])
    free = [c for c in range(len(mb)) if c not in (3, 4)]
    rows = {}
    # rows with an all-zero reference set of n > 32 (own value > 0 -> z = +inf; own value 0 below)
    zrows = []
    for j, nz in enumerate(ZERO_N):
        if nz > k:
            continue
        for i in (int(start[free[6 + j]]) + 3, gstart + 7 + j, B - 1 - j):
            idx[i, :nz] = [cd(jj, chrom(i)) for jj in Z[:nz]]
            dist[i, :nz] = 0.01
            dist[i, nz:] = FAR
            zrows.append(i)
    rows["zero_ref"] = zrows
    # rows with exactly m selected reference bins (m = 0, 1, 2, 32, 33, k)
    srows = []
    for j, m in enumerate(NSEL + (k,)):
        if m > k:
            continue
        for i in (int(start[free[1 + j]]) + 11, gstart + 20 + j):
            pos = rng.permutation(k)[:m]
            dist[i, :] = FAR
            dist[i, pos] = rng.uniform(0.01, 0.2, m)
            srows.append(i)
    rows["nsel"] = srows
    # padding rows: trailing idx = -1 / dist = 1e10 (fewer candidates than k); one all padding
    prows = []
    for j, p in enumerate((1, min(17, k), k)):
        for i in (int(start[free[9 + j]]) + 2, gstart + 30 + j):
            idx[i, k - p:] = -1
            dist[i, k - p:] = 1e10
            prows.append(i)
    rows["padding"] = prows
    ref = {"indexes": idx, "distances": dist, "masked_bins_per_chr": mb,
           "masked_bins_per_chr_cum": cum}
    info = {"B": B, "k": k, "Z": Z, "Z2": Z2, "rows": rows, "ct_g": gstart, "free": free,
            "start": start}
    return ref, info


def make_samples(info, ns, seed, dead=None):
    """ns samples around 1 with both zero stretches; the samples at PLANT_AT and the last one get
    heavy tails (1e6x), NaN, negative values, an integer-valued stretch (ties, even middles), a gain
    and a zero stretch of their own; sample `dead` is all negative (every row at n = 0)."""
    rng = np.random.default_rng(seed)
    B, start, free = info["B"], info["start"], info["free"]
    xs = 1.0 + 0.05 * rng.standard_normal((ns, B))
    xs[:, info["Z"]] = 0.0
    xs[:, info["Z2"]] = 0.0
    keep_out = set(info["Z"]) | set(info["Z2"])
    pool = np.array([i for i in range(B) if i not in keep_out])
    for s in sorted({p for p in PLANT_AT if p < ns} | {ns - 1}):
        x = xs[s]
        x[rng.choice(pool, 4, replace=False)] *= 1e6                       # heavy tails
        x[rng.choice(pool, 3, replace=False)] = np.nan
        x[rng.choice(pool, 5, replace=False)] = -rng.uniform(0.1, 2.0, 5)    # dropped by >= 0
        c = free[(s % 7) + 2]
        a = int(start[c]) + 1
        x[a:a + 30] = rng.integers(0, 4, 30).astype(np.float64)             # integer stretch
        c = free[(s % 5) + 12]
        a = int(start[c]) + 1
        x[a:a + 12] = 0.0                                                   # zero stretch
        x[a + 12:a + 20] *= 1.6                                             # gain
        # a large share of integer values over the whole sample: reference sets with ties
        q = rng.choice(pool, B // 3, replace=False)
        x[q] = np.round(x[q] * 4.0) / 4.0
    if dead is not None and dead < ns:
        xs[dead] = -1.0
    return xs


# (k, n_samples, layout, cut-off) of every case; A: ct = 0; Gs / Gb: the gonosomal pass (ct = first
# bin of chromosome 23, cp = 22) with small gonosomes / with gonosomes holding a quarter of the bins
CASES = [
    # one sample
    (1, 1, "A", CUT), (65, 1, "Gb", WIDE), (200, 1, "A", CUT), (448, 1, "Gs", CUT),
    (129, 1, "Gs", CUT), (320, 1, "Gb", CUT), (384, 1, "A", WIDE), (512, 1, "A", CUT),
    (513, 1, "A", WIDE), (1024, 1, "Gb", CUT), (2048, 1, "A", CUT),
    # 2..15 samples: tiled kernel
    (63, 2, "A", CUT), (128, 8, "Gb", CUT), (129, 9, "A", WIDE), (200, 8, "Gs", CUT),
    (320, 15, "Gs", CUT), (384, 15, "A", CUT), (448, 2, "Gb", CUT), (512, 9, "A", CUT),
    # 16..128 samples, rank medians (ct = 0, or gonosomes >= 1/4 of the bins)
    (1, 16, "A", CUT), (64, 17, "Gb", CUT), (128, 64, "A", WIDE), (129, 65, "Gb", CUT),
    (200, 128, "A", CUT), (256, 16, "Gb", CUT), (320, 17, "A", CUT), (384, 64, "Gb", CUT),
    (448, 65, "A", WIDE), (511, 128, "Gb", CUT), (512, 16, "A", CUT),
    # 16..128 samples, small gonosomes: lanes + incremental, tiled last pass
    (63, 16, "Gs", CUT), (129, 128, "Gs", CUT), (256, 64, "Gs", WIDE), (512, 65, "Gs", CUT),
    # more than 128 samples: lanes + incremental, tiled last pass
    (65, 129, "A", CUT), (384, 129, "Gs", CUT), (511, 129, "Gb", WIDE),
    # k > 512, 2 samples and more: one-sample kernel, a grid row per sample
    (513, 2, "Gb", CUT), (1024, 9, "A", CUT), (1025, 16, "Gs", WIDE), (2048, 2, "Gb", CUT),
]
# one sample with every row at n = 0 on its own (the one-sample nanmedian); batches of 3 and more
# carry such a sample at position 1 (k_nanmedian)
DEAD_SINGLE = (65, 1, "A", CUT)


def case_ct(info, lay):
    return (info["ct_g"], 22) if lay != "A" else (0, 0)


def case_id(case):
    k, ns, lay, cut = case
    B = int(layout(k, lay).sum())
    ct = int(layout(k, lay)[:22].sum()) if lay != "A" else 0
    return "%s-k%d-n%d-%s-%s" % (norm_path(k, ns, B, ct), k, ns, lay, "wide" if cut == WIDE else "cut")
