"""Host references for tn_pair_rowsums and tnac4o.calculate_overlap_errors (numpy and Python integers, no GPU).

- pair_rowsums_ref: the six sums of every row by brute force over the distance matrix of overlap_ref.pair_dist_ref, in Python integers.
- moments_ref: the overlap moments of a set of samples by the trusted path, overlap_ref.distribution_ref + overlap.moments.
- jackknife_ref: the delete-one jackknife recomputed from scratch -- moments_ref on the M - 1 remaining samples, once per sample.
- class_rowsums: the input of overlap.jackknife (R, wq, scale, inv) for given samples, with the integers taken from pair_rowsums_ref.
"""
import numpy as np

import overlap_ref as oref


def pair_rowsums_ref(rows, nbits, w=None, lanes16=False, dist=None):
    """M lists of six Python integers: for row a and over every b != a with d = dist(a, b),
    [sum w_b, sum w_b d, sum w_b d^2, sum w_b d^3, sum w_b d^4, sum w_b |nbits - 2 d|].  w: None (all 1) or M integers."""
    D = (oref.pair_dist_ref(rows, nbits, lanes16) if dist is None else dist).astype(object)
    M = D.shape[0]
    if M == 0:
        return []
    wv = np.array([1] * M if w is None else [int(x) for x in w], dtype=object)
    W = np.tile(wv, (M, 1))
    np.fill_diagonal(W, 0)                                             # the row itself does not enter
    WD2 = W * D * D
    fold = np.array([[abs(nbits - 2 * d) for d in row] for row in D], dtype=object).reshape(M, M)
    cols = [W, W * D, WD2, WD2 * D, WD2 * D * D, W * fold]
    return [[int(c[a].sum()) for c in cols] for a in range(M)]


def limbs(R):
    """M lists of six Python integers -> (M, 6, 2) uint64 (lo, hi)."""
    return oref.limbs([v for row in R for v in row]).reshape(len(R), 6, 2)


def moments_ref(X, w, kind):
    """The overlap moments of the samples X (M, n) with weights w from all ordered pairs in float64, by the path the overlap tests
    trust: distribution_ref, then overlap.moments (and chi_sg = n q2 for 'spin')."""
    from tnac4o_amd import overlap
    values, P = oref.distribution_ref(X, w, kind)
    m = overlap.moments(values, P)
    if kind == 'spin':
        m['chi_sg'] = X.shape[1] * m['q2']
    return m


def jackknife_ref(X, w, kind):
    """(estimate, leave_one_out, error, bias_corrected): moments_ref on all samples with w > 0 and on the M' - 1 that remain without
    each of them in turn; leave_one_out[key] is (M,), nan where w_s = 0."""
    X, w = np.asarray(X), np.asarray(w, dtype=np.float64)
    M = X.shape[0]
    est = moments_ref(X, w, kind)
    loo = {k: np.full(M, np.nan) for k in est}
    for s in np.flatnonzero(w > 0):
        rest = np.arange(M) != s
        for k, v in moments_ref(X[rest], w[rest], kind).items():
            loo[k][s] = v
    Mp = int(np.count_nonzero(w > 0))
    err, corr = {}, {}
    for k in est:
        v = loo[k][w > 0]
        err[k] = float(np.sqrt((Mp - 1.0) / Mp * np.sum((v - v.mean()) ** 2)))
        corr[k] = Mp * est[k] - (Mp - 1.0) * float(v.mean())
    return est, loo, err, corr


def class_rowsums(X, w, kind):
    """(R, wq, scale, inv, n): what overlap.jackknife takes for the samples X (M, n) -- bits for 'spin' and 'link', cell states in
    [0, 32768) for 'cell' -- with weights w: overlap.prepare_with_inverse, and pair_rowsums_ref on the kept distinct rows."""
    from tnac4o_amd import overlap
    X = np.asarray(X)
    lanes16 = kind == 'cell'
    rows = overlap.pack_lanes16(X) if lanes16 else overlap.pack_bits(X)
    urows, wq, scale, _, inv = overlap.prepare_with_inverse(rows, np.asarray(w, dtype=np.float64))
    return pair_rowsums_ref(urows, X.shape[1], wq, lanes16), wq, scale, inv, int(X.shape[1])
