"""Replica-overlap distributions of a set of configurations (host side of tnac4o.calculate_overlap_distribution) and
their line-resolved second moments (tnac4o.calculate_overlap_correlations), and the correlations of every pair of spins
over the configurations (tnac4o.calculate_sample_correlations), and the jackknife errors of the overlap moments
(tnac4o.calculate_overlap_errors).

Plain numpy, importable without a GPU; the only device work is the pair histogram tn_pair_hist (ops.pair_hist), which the driver
overlap_distribution calls once, the pair moments tn_pair_moments (ops.pair_moments), which overlap_correlations calls once per axis,
the spin moments tn_spin_moments (ops.spin_moments), which sample_correlations calls once, and the per-row sums tn_pair_rowsums
(ops.pair_rowsums), which overlap_errors calls once.  Row layouts of the library: a row of
n bits is ceil(n / 64) uint64 words, bit i in word i // 64 at position i % 64; a row of n 16-bit lanes is ceil(n / 4) words, lane i
in word i // 4 at bits 16 (i % 4) .. 16 (i % 4) + 15."""
import numpy as np

MAX_NBITS = 9183                 # largest row tn_pair_hist takes: 16 bytes per bin and the staging in 160 KiB of LDS (include/tnpeps.h)
WMAX = 2 ** 32 - 1               # weights of tn_pair_hist are uint32
KINDS = ('spin', 'link', 'cell')


# ---------------------------------------------------------------------------------------------- packing
def pack_bits(bits):
    """(M, n) array of 0 / 1 -> (M, ceil(n / 64)) uint64."""
    bits = np.asarray(bits)
    if bits.ndim != 2:
        raise ValueError('bits must be a 2-d array')
    if bits.size and not np.all((bits == 0) | (bits == 1)):
        raise ValueError('bits must be 0 or 1')
    M, n = bits.shape
    nwords = -(-n // 64)
    by = np.zeros((M, nwords * 8), dtype=np.uint8)
    if n:
        pk = np.packbits(bits.astype(np.uint8), axis=1, bitorder='little')
        by[:, :pk.shape[1]] = pk
    return np.ascontiguousarray(by).view('<u8').astype(np.uint64, copy=False)


def pack_lanes16(states):
    """(M, n) array of cell states in [0, 32768) -> (M, ceil(n / 4)) uint64, four 16-bit lanes per word."""
    states = np.asarray(states)
    if states.ndim != 2:
        raise ValueError('states must be a 2-d array')
    if states.size and (states.min() < 0 or states.max() >= 32768):
        raise ValueError('cell states must lie in [0, 32768)')
    M, n = states.shape
    nwords = -(-n // 4)
    la = np.zeros((M, nwords * 4), dtype='<u2')
    la[:, :n] = states
    return np.ascontiguousarray(la).view('<u8').astype(np.uint64, copy=False)


def link_pairs(J0):
    """The couplings of an Ising model: every i < j with off-diagonal J0[i, j] != 0, sorted -- the bond_pairs of model_correlations."""
    return np.argwhere(np.triu(np.asarray(J0), 1) != 0).astype(np.int64)


def _ising(solver, what):
    if solver.mode != 'Ising':
        raise ValueError("%s is defined for mode 'Ising' only" % what)


def active_spins(solver):
    """The spins the cells of solver.ind0 list, sorted: int64."""
    return np.sort(np.concatenate([np.asarray(a, dtype=np.int64) for row in solver.ind0 for a in row] + [np.zeros(0, dtype=np.int64)]))


def spin_bits(solver):
    """binary_states() of solver.states restricted to the active spins, in model order: (M, solver.active) of 0 / 1.  Ising only."""
    _ising(solver, 'spin_bits')
    return solver.binary_states()[:, active_spins(solver)].astype(np.uint8)


def link_bits(solver):
    """One bit per coupling of solver.states, [s_i == s_j], couplings in the order of link_pairs(solver.J0); from J0 alone.  Ising only."""
    _ising(solver, 'link_bits')
    pairs = link_pairs(solver.J0)
    b = solver.binary_states()
    return (b[:, pairs[:, 0]] == b[:, pairs[:, 1]]).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- estimator
def condense(rows, w):
    """Distinct rows with their aggregated weights.  rows (M, nwords) uint64, w (M,) -> (urows (K, nwords), W (K,) summed weights,
    D0): D0 = sum_c (W_c^2 - S_c) / 2 with S_c the summed squared weights is the weight of the pairs of DISTINCT samples that carry
    the SAME row: they have distance 0 and belong to bin 0.  float64 throughout.  The pair histogram of all M rows equals the one of
    the K distinct rows with weights W plus D0 in bin 0; at low temperature, where one row carries most of the weight, this keeps
    those pairs off a single word of the device histogram."""
    return condense_with_inverse(rows, w)[:3]


def condense_with_inverse(rows, w):
    """condense, and the class of every sample: (urows, W, D0, inv) with inv (M,) int64, rows[s] == urows[inv[s]]."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    w = np.asarray(w, dtype=np.float64)
    if rows.ndim != 2 or w.shape != (rows.shape[0],):
        raise ValueError('rows (M, nwords) and w (M,) expected')
    if rows.shape[0] == 0:
        return rows, w, 0.0, np.zeros(0, dtype=np.int64)
    if rows.shape[1] == 0:
        urows, inv = rows[:1], np.zeros(rows.shape[0], dtype=np.int64)
    else:
        urows, inv = np.unique(rows, axis=0, return_inverse=True)
    inv = np.asarray(inv).reshape(-1).astype(np.int64, copy=False)
    W = np.bincount(inv, weights=w, minlength=urows.shape[0])
    S = np.bincount(inv, weights=w * w, minlength=urows.shape[0])
    return urows, W, float(np.sum(W * W - S) / 2.0), inv


def quantise(W, wmax=WMAX):
    """Weights as the uint32 tn_pair_hist takes: (wq (K,) uint32, keep (K,) bool, scale) with wq = rint(scale * W).  Integer W up to
    2^32 - 1 (the multiplicities under uniform weights) pass through with scale 1: the device result is then the exact pair count.
    Otherwise two scales are tried, (2^32 - 1) / max W and the largest power of two below it, and the one with the smaller total
    rounding error sum |wq / scale - W| is taken.  The first puts every weight within half a unit, 2^-33 of the largest, so the
    total is at most K 2^-33 max W with either.  The second is exact for weights that are multiples of a common power of two up to
    rounding -- multiplicities of nearly equal importance weights -- where the first would shift every row of one multiplicity by
    the same amount.  keep marks the rows with wq > 0; the others are to be dropped.  wmax: the largest quantised weight, in place
    of 2^32 - 1 everywhere above (tn_pair_moments takes less, so that its products stay below 2^64)."""
    W = np.asarray(W, dtype=np.float64)
    wmax = int(wmax)
    if not 1 <= wmax <= WMAX:
        raise ValueError('wmax must lie in 1 .. 2^32 - 1')
    if W.size == 0:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=bool), 1.0
    if np.all(W == np.rint(W)) and W.max() <= wmax:
        wq, scale = W, 1.0
    else:
        full = wmax / float(W.max())
        best = None
        for sc in (full, 2.0 ** np.floor(np.log2(full))):
            q = np.minimum(np.rint(W * sc), wmax)
            err = float(np.sum(np.abs(q / sc - W)))
            if best is None or err < best[0]:
                best = (err, q, sc)
        _, wq, scale = best
    wq = wq.astype(np.uint32)
    return wq, wq > 0, float(scale)


def prepare(rows, w, wmax=WMAX):
    """(urows, wq, scale, D0): condense, then quantise with wmax; only the distinct rows that keep a weight wq > 0, contiguous."""
    urows, W, D0 = condense(rows, w)
    wq, keep, scale = quantise(W, wmax)
    return np.ascontiguousarray(urows[keep]), np.ascontiguousarray(wq[keep]), scale, D0


def prepare_with_inverse(rows, w, wmax=WMAX):
    """prepare, and where every sample went: (urows, wq, scale, D0, inv) with inv (M,) int64 = the index of sample s's row among the
    kept distinct rows, -1 when the quantisation dropped it."""
    urows, W, D0, inv = condense_with_inverse(rows, w)
    wq, keep, scale = quantise(W, wmax)
    index = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
    return np.ascontiguousarray(urows[keep]), np.ascontiguousarray(wq[keep]), scale, D0, index[inv] if inv.size else inv


def upload(urows, wq):
    """(d_rows, d_w) on the device; d_w = None when every weight is 1."""
    import torch
    return torch.as_tensor(urows.view(np.int64)).cuda(), None if np.all(wq == 1) else torch.as_tensor(wq.view(np.int32)).cuda()


def limbs_to_int(hist_limbs):
    """(nbins, 2) limbs (lo, hi; any integer dtype, read as unsigned 64-bit) -> list of Python ints lo + 2^64 hi."""
    h = np.asarray(hist_limbs)
    if h.dtype != object:
        h = np.ascontiguousarray(h).astype(np.int64, copy=False).view(np.uint64)
    return [int(lo) + (int(hi) << 64) for lo, hi in h]


def distribution(hist_limbs, scale, D0):
    """P over the bins, float64, normalised to 1: (hist / scale^2 + D0 [d = 0]) / total, hist the integers of the device histogram of
    the condensed rows, D0 the self term of condense in units of the unquantised weights."""
    H = np.array([float(v) for v in limbs_to_int(hist_limbs)], dtype=np.float64) / (float(scale) * float(scale))
    H[0] += D0
    total = H.sum()
    if not total > 0:
        raise ValueError('no pair of distinct samples carries weight')
    return H / total


def moments(values, P):
    """<q>, <|q|>, <q^2>, <q^4> and the Binder ratio (3 - <q^4> / <q^2>^2) / 2 of the distribution P over `values`."""
    q, P = np.asarray(values, dtype=np.float64), np.asarray(P, dtype=np.float64)
    q2, q4 = float(P @ q ** 2), float(P @ q ** 4)
    return {'q': float(P @ q), 'abs_q': float(P @ np.abs(q)), 'q2': q2, 'q4': q4, 'binder': 0.5 * (3.0 - q4 / (q2 * q2)) if q2 > 0 else float('nan')}


def effective_sample_size(w):
    """(sum w)^2 / sum w^2 of the raw weights."""
    w = np.asarray(w, dtype=np.float64)
    return float(w.sum() ** 2 / np.sum(w * w))


def overlap_values(kind, n):
    """The overlap at distance d = 0 .. n: 1 - 2 d / n for 'spin' and 'link', the fraction of equal cells 1 - d / n for 'cell'."""
    d = np.arange(n + 1, dtype=np.float64)
    return 1.0 - (1.0 if kind == 'cell' else 2.0) * d / n


# ---------------------------------------------------------------------------------------------- driver
def check_arguments(solver, kind, weights):
    """Everything calculate_overlap_distribution can refuse before any device work.  Returns (kind, w (M,) float64)."""
    if kind is None:
        kind = 'spin' if solver.mode == 'Ising' else 'cell'
    if kind not in KINDS:
        raise ValueError("kind must be 'spin', 'link', 'cell' or None")
    if kind != 'cell' and solver.mode != 'Ising':
        raise ValueError("kind '%s' is defined for mode 'Ising' only" % kind)
    M = int(np.asarray(solver.states).shape[0])
    if M < 2:
        raise ValueError('calculate_overlap_distribution needs at least two stored states (run sample_boltzmann, gibbs_sampling, a search or '
                         'decode_low_energy_states first)')
    if isinstance(weights, str):
        if weights == 'uniform':
            w = np.ones(M)
        elif weights == 'importance':
            lz = getattr(solver, 'sample_log2Z', None)
            if lz is None or np.asarray(lz).shape != (M,):
                raise ValueError("weights='importance' needs sample_log2Z of the stored states: run sample_boltzmann first")
            lz = np.asarray(lz, dtype=np.float64)
            if not np.all(np.isfinite(lz)):
                raise ValueError('sample_log2Z is not finite')
            w = np.exp2(lz - lz.max())
        else:
            raise ValueError("weights must be 'uniform', 'importance' or an array of length M")
    else:
        try:
            w = np.array(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('weights must be numbers') from None
        if w.shape != (M,):
            raise ValueError('weights must have length %d, the number of stored states' % M)
        if not np.all(np.isfinite(w)) or np.any(w < 0):
            raise ValueError('weights must be non-negative and finite')
        if not w.max() > 0:
            raise ValueError('all weights are zero')
    return kind, w


def cell_states(solver):
    """solver.states with the cell states read as unsigned: the solver keeps 256 states of a cell in int8."""
    st = np.asarray(solver.states)
    return st.view('u%d' % st.dtype.itemsize) if st.dtype.kind == 'i' and st.dtype.itemsize < 8 else st


def rows_of(solver, kind):
    """(packed rows (M, nwords) uint64, n, lanes16) of solver.states for a kind."""
    if kind == 'cell':
        st = cell_states(solver)
        return pack_lanes16(st), int(st.shape[1]), True
    bits = spin_bits(solver) if kind == 'spin' else link_bits(solver)
    return pack_bits(bits), int(bits.shape[1]), False


def overlap_distribution(solver, kind=None, weights='uniform'):
    """calculate_overlap_distribution of tnac4o (documented there)."""
    kind, w = check_arguments(solver, kind, weights)
    rows, n, lanes16 = rows_of(solver, kind)
    if n < 1:
        raise ValueError("kind '%s': the model has nothing to compare" % kind)
    if n > MAX_NBITS:
        raise NotImplementedError("kind '%s' compares %d %s per state; tn_pair_hist takes at most %d (its histogram must fit the 160 KiB of "
                                  'LDS); there is no host fallback' % (kind, n, 'cells' if lanes16 else 'bits', MAX_NBITS))
    from . import ops
    urows, wq, scale, D0 = prepare(rows, w)
    if urows.shape[0] >= 2:
        d_rows, d_w = upload(urows, wq)
        limbs = ops.pair_hist(d_rows, n, d_w, lanes16).cpu().numpy()
    else:                                            # one distinct row: every pair sits in D0
        limbs = np.zeros((n + 1, 2), dtype=np.int64)
    P = distribution(limbs, scale, D0)
    solver.overlap_kind = kind
    solver.overlap_values = overlap_values(kind, n)
    solver.overlap_distribution = P
    solver.overlap_moments = moments(solver.overlap_values, P)
    if kind == 'spin':
        solver.overlap_moments['chi_sg'] = n * solver.overlap_moments['q2']
    solver.overlap_ess = effective_sample_size(w)
    solver.overlap_pairs = rows.shape[0] * (rows.shape[0] - 1) // 2
    return P


# ---------------------------------------------------------------------------------------------- jackknife errors
MAX_ROWSUM_NBITS = 65535         # largest row tn_pair_rowsums takes: w d^2 below 2^64, a row's sum of w d^4 below 2^127 (include/tnpeps.h)
_SLOT_POWER = (0, 1, 1, 2, 4)    # the slots of a row's moments: k = 0, 1, A (|q|), 2, 4 and the power of n that an equal row contributes


def rowsums_to_int(limbs):
    """(K, 6, 2) limbs of tn_pair_rowsums (lo, hi; any integer dtype, read as unsigned 64-bit) -> K lists of six Python ints."""
    h = np.asarray(limbs)
    if h.ndim != 3 or h.shape[1:] != (6, 2):
        raise ValueError('limbs (K, 6, 2) expected')
    flat = limbs_to_int(h.reshape(-1, 2))
    return [flat[6 * a:6 * a + 6] for a in range(h.shape[0])]


def _row_moments(R, n, kind):
    """For every row a the integers sum_{b != a} wq_b (n - c d_ab)^k in the slots k = 0, 1, A, 2, 4, from R_a[0 .. 5] by the binomial
    expansion in Python integers (slot A: R_a[5] = sum wq_b |n - 2 d| for 'spin' and 'link'; for 'cell' |q| = q, the slot of k = 1)."""
    c = 1 if kind == 'cell' else 2
    out = []
    for R0, R1, R2, R3, R4, R5 in ([int(v) for v in row] for row in R):
        I1 = n * R0 - c * R1
        I2 = n * n * R0 - 2 * n * c * R1 + c * c * R2
        I4 = n ** 4 * R0 - 4 * n ** 3 * c * R1 + 6 * n * n * c * c * R2 - 4 * n * c ** 3 * R3 + c ** 4 * R4
        out.append((R0, I1, I1 if kind == 'cell' else R5, I2, I4))
    return out


def _theta(Q, n, spin):
    """The estimates from the five pair sums Q (slots 0, 1, A, 2, 4; any common factor cancels): dict over the keys of overlap_moments;
    nan throughout when no pair carries weight."""
    keys = ('q', 'abs_q', 'q2', 'q4', 'binder') + (('chi_sg',) if spin else ())
    if not Q[0] > 0:
        return dict.fromkeys(keys, float('nan'))
    q2, q4 = Q[3] / (n * n * Q[0]), Q[4] / (n ** 4 * Q[0])
    t = {'q': Q[1] / (n * Q[0]), 'abs_q': Q[2] / (n * Q[0]), 'q2': q2, 'q4': q4, 'binder': 0.5 * (3.0 - q4 / (q2 * q2)) if q2 > 0 else float('nan')}
    if spin:
        t['chi_sg'] = n * q2
    return t


def jackknife(R, wq, scale, inv, w, n, kind):
    """Delete-one jackknife of the overlap moments of M weighted samples (calculate_overlap_errors of tnac4o).
    R: K rows of six integers, the sums of tn_pair_rowsums over the K kept distinct rows (rowsums_to_int); wq (K,), scale: their
    quantised weights (prepare); inv (M,): the kept row of sample s, -1 when the quantisation dropped it; w (M,): the raw weights;
    n: bits (cells) per row; kind: 'spin', 'link' or 'cell'.
    With c = 2 ('cell': 1) and What_b = wq_b / scale: r_a[k] = sum_{b != a} What_b (n - c d_ab)^k for k = 0, 1, 2, 4 and
    r_a[A] = sum What_b |n - 2 d_ab| ('cell': r_a[1]); W_c = the summed raw weight of the samples that carry row c;
    Q_k = 1/2 sum_s w_s (r_c(s)[k] + (W_c(s) - w_s) n^k), the second term for the other samples with the same row (A: n^1).
    q = Q_1 / (n Q_0), abs_q = Q_A / (n Q_0), q2 = Q_2 / (n^2 Q_0), q4 = Q_4 / (n^4 Q_0), binder = (3 - q4 / q2^2) / 2, chi_sg = n q2
    ('spin' only).  Without sample s: Q_k - w_s (r_c(s)[k] + (W_c(s) - w_s) n^k), and theta^(-s) from the same formulas; a sample of a
    dropped row leaves theta as it is.  Only samples with w_s > 0 count, M' of them (fewer than three: ValueError).  With tbar the
    mean of theta^(-s): error = sqrt((M' - 1) / M' sum_s (theta^(-s) - tbar)^2), bias_corrected = M' theta - (M' - 1) tbar.
    The binomial sums are always formed in Python integers; with scale 1 and integer raw weights everything up to the final
    divisions is (then theta^(-s) is computed once per distinct (row, weight): K values under uniform weights); otherwise the
    integers are divided by scale and the rest is float64, the sums over the samples without rounding (math.fsum).  Rounded
    weights: in the first term w_s stands for w_s What_c / W_c, the sample's share of the ROUNDED weight of its row (a factor within
    2^-33 max W / W_c of 1), so that Q_k is the pair sum of `distribution` -- hist / scale^2 + D0 -- to rounding and the estimate
    is that of calculate_overlap_distribution; the second term keeps the raw weights, as D0 does.
    Returns {'estimate', 'error', 'bias_corrected', 'leave_one_out'}, each a dict over the keys of overlap_moments (leave_one_out:
    arrays (M,), nan where w_s = 0), and 'state_q', 'state_q2' (M,): the mean of q and q^2 of state s with all OTHER samples,
    (r[1] + (W_c - w_s) n) / (n (r[0] + W_c - w_s)) and likewise with r[2] and n^2 (nan for a dropped row or without partners)."""
    import math
    from collections import Counter
    if kind not in KINDS:
        raise ValueError("kind must be 'spin', 'link' or 'cell'")
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    inv = np.asarray(inv, dtype=np.int64).reshape(-1)
    wq = np.asarray(wq).reshape(-1)
    n, M, K = int(n), w.size, wq.size
    if inv.shape != (M,) or len(R) != K or n < 1 or inv.size and (inv.min() < -1 or inv.max() >= K):
        raise ValueError('R and wq of the K kept rows, inv and w of the M samples expected')
    counted = w > 0
    Mp = int(np.count_nonzero(counted))
    if Mp < 3:
        raise ValueError('the jackknife needs at least three samples with a positive weight')
    spin = kind == 'spin'
    I = _row_moments(R, n, kind)
    powers = [n ** p for p in _SLOT_POWER]
    exact = float(scale) == 1.0 and bool(np.all(w == np.rint(w)))
    if exact:
        r, Wc, ws, g, total = I, [int(x) for x in wq], [int(x) for x in w], [1] * K, sum
    else:
        r = [tuple(float(v) / float(scale) for v in row) for row in I]
        Wc = np.bincount(inv[inv >= 0], weights=w[inv >= 0], minlength=K).tolist()
        ws = w.tolist()
        g = [float(q) / float(scale) / W if W > 0 else 0.0 for q, W in zip(wq.tolist(), Wc)]        # What_c / W_c
        total = math.fsum
    cls = inv.tolist()
    # what a sample contributes to 2 Q, once per distinct (row, weight)
    share = {}
    for key in set(zip(cls, ws)):
        c, x = key
        if c >= 0:
            share[key] = tuple(x * g[c] * r[c][k] + x * (Wc[c] - x) * powers[k] for k in range(5))
    count = Counter(zip(cls, ws))
    Q2 = [total(count[key] * t[k] for key, t in share.items()) for k in range(5)]
    theta = _theta(Q2, n, spin)
    if theta['q'] != theta['q']:
        raise ValueError('no pair of distinct samples carries weight')
    keys = list(theta)
    loo_of, state_of = {}, {}
    for key, t in share.items():
        c, x = key
        loo_of[key] = _theta([Q2[k] - 2 * t[k] for k in range(5)], n, spin) if x > 0 else None
        den = r[c][0] + Wc[c] - x
        state_of[key] = ((r[c][1] + (Wc[c] - x) * n) / (n * den), (r[c][3] + (Wc[c] - x) * n * n) / (n * n * den)) if den > 0 else (float('nan'),) * 2
    loo = {k: np.full(M, np.nan) for k in keys}
    state_q, state_q2 = np.full(M, np.nan), np.full(M, np.nan)
    for s, key in enumerate(zip(cls, ws)):
        if key in share:
            state_q[s], state_q2[s] = state_of[key]
        if key[1] > 0:
            t = loo_of[key] if key in share else theta
            for k in keys:
                loo[k][s] = t[k]
    est, err, corr = {}, {}, {}
    for k in keys:
        v = loo[k][counted]
        tbar = float(np.mean(v))
        est[k] = float(theta[k])
        err[k] = float(np.sqrt((Mp - 1.0) / Mp * np.sum((v - tbar) ** 2)))
        corr[k] = Mp * est[k] - (Mp - 1.0) * tbar
    return {'estimate': est, 'error': err, 'bias_corrected': corr, 'leave_one_out': loo, 'state_q': state_q, 'state_q2': state_q2}


def overlap_errors(solver, kind=None, weights='uniform'):
    """calculate_overlap_errors of tnac4o (documented there)."""
    kind, w = check_arguments(solver, kind, weights)
    if np.count_nonzero(w > 0) < 3:
        raise ValueError('calculate_overlap_errors needs at least three stored states with a positive weight')
    rows, n, lanes16 = rows_of(solver, kind)
    if n < 1:
        raise ValueError("kind '%s': the model has nothing to compare" % kind)
    if n > MAX_ROWSUM_NBITS:
        raise NotImplementedError("kind '%s' compares %d %s per state; tn_pair_rowsums takes at most %d (its sums of w d^4 must stay below "
                                  '2^127); there is no host fallback' % (kind, n, 'cells' if lanes16 else 'bits', MAX_ROWSUM_NBITS))
    urows, wq, scale, _, inv = prepare_with_inverse(rows, w)
    if urows.shape[0] >= 2:
        from . import ops
        d_rows, d_w = upload(urows, wq)
        limbs = ops.pair_rowsums(d_rows, n, d_w, lanes16).cpu().numpy()
    else:                                            # one distinct row: no pair of distinct rows, every sum is zero
        limbs = np.zeros((urows.shape[0], 6, 2), dtype=np.int64)
    jk = jackknife(rowsums_to_int(limbs), wq, scale, inv, w, n, kind)
    solver.overlap_errors = jk['error']
    solver.overlap_error_estimates = jk['estimate']
    solver.overlap_bias_corrected = jk['bias_corrected']
    solver.overlap_state_q = jk['state_q']
    solver.overlap_state_q2 = jk['state_q2']
    solver.overlap_error_kind = kind
    solver.overlap_ess = effective_sample_size(w)
    return jk['error']


# ---------------------------------------------------------------------------------------------- line-resolved overlaps
MAX_GROUPS = 64                  # lattice columns (rows) tn_pair_moments takes: the distance table of 65 groups fills the 160 KiB of LDS
MAX_GROUP_WORDS = 32             # words of one group: 2048 spins or 128 cells in a lattice column (row)


def line_groups(solver, axis, kind):
    """The lattice line of everything a state is compared by: (group (n,) int64, sizes (G,) int64).  kind 'spin': entry k belongs to bit
    k of spin_bits(solver), an active spin in model order; kind 'cell': to cell k of `states` (model cell order, k = ny Nx + nx).
    The group is the model column nx (axis 'x', G = Nx) or the model row ny (axis 'y', G = Ny) of the cell -- for a spin, of the cell
    that lists it in solver.ind0[ny][nx].  sizes[g] = the number of entries of group g."""
    if axis not in ('x', 'y'):
        raise ValueError("axis must be 'x' or 'y'")
    if kind not in ('spin', 'cell'):
        raise ValueError("kind must be 'spin' or 'cell' (a coupling lies in two groups)")
    Nx, Ny = int(solver.Nx_model), int(solver.Ny_model)
    line = np.tile(np.arange(Nx), Ny) if axis == 'x' else np.repeat(np.arange(Ny), Nx)           # of cell k = ny Nx + nx
    if kind == 'cell':
        group = line.astype(np.int64)
    else:
        _ising(solver, "kind 'spin'")
        cell = {int(i): ny * Nx + nx for ny, row in enumerate(solver.ind0) for nx, a in enumerate(row) for i in a}
        group = line[[cell[int(i)] for i in active_spins(solver)]].astype(np.int64)              # in the order of spin_bits
    return group, np.bincount(group, minlength=Nx if axis == 'x' else Ny).astype(np.int64)


def pack_groups(bits_or_states, group, G, lanes16):
    """(M, n) bits (lanes16: cell states in [0, 32768)) with the group of every column -> (rows (M, G wpg) uint64, wpg): group g in
    the words [g wpg, (g+1) wpg) of a row, its entries in the order of their columns, layout of pack_bits (pack_lanes16) within the
    group, zeros behind them.  wpg = the words of the largest group, at least 1."""
    X = np.asarray(bits_or_states)
    group = np.asarray(group, dtype=np.int64).reshape(-1)
    G = int(G)
    if X.ndim != 2 or group.shape != (X.shape[1],):
        raise ValueError('an (M, n) array and the group of each of its n columns expected')
    if G < 1 or group.size and (group.min() < 0 or group.max() >= G):
        raise ValueError('groups must lie in [0, G)')
    per = 4 if lanes16 else 64
    sizes = np.bincount(group, minlength=G)
    wpg = max(1, -(-int(sizes.max()) // per))
    order = np.argsort(group, kind='stable')
    rank = np.empty(group.size, dtype=np.int64)
    rank[order] = np.arange(group.size) - np.concatenate([[0], np.cumsum(sizes)])[group[order]]  # position within the group
    wide = np.zeros((X.shape[0], G * wpg * per), dtype=np.int64)
    wide[:, group * (wpg * per) + rank] = X
    return (pack_lanes16(wide) if lanes16 else pack_bits(wide)), wpg


def second_moments(out_limbs, sizes, kind, scale=1.0, D0=0.0):
    """(<Q_g> (G,), <Q_g Q_g'> (G, G)) in float64 from the integers of tn_pair_moments: out_limbs (G+1, G+1, 2), sizes n_g, Q_g =
    n_g - 2 d_g for 'spin' (the sum of s_a s_b over the group) and n_g - d_g for 'cell' (the equal cells).  With c = 2 or 1,
    sum p Q_g Q_g' = n_g n_g' out[G][G] - c n_g out[g'][G] - c n_g' out[g][G] + c^2 out[g][g'] is formed in Python integers and
    divided once by sum p = out[G][G], so the cancellation is exact.  D0 (condense) is the weight of the pairs of equal rows, in
    units of the unquantised weights: they have d_g = 0 for every g, so Q_g = n_g, and enter both sums -- as an integer when the
    weights are integers (scale 1), as a float otherwise."""
    h = np.asarray(out_limbs)
    G = h.shape[0] - 1
    n = [int(x) for x in sizes]
    if h.shape != (G + 1, G + 1, 2) or len(n) != G:
        raise ValueError('out_limbs (G+1, G+1, 2) and G sizes expected')
    O = limbs_to_int(h.reshape(-1, 2))
    O = [O[i * (G + 1):(i + 1) * (G + 1)] for i in range(G + 1)]
    c = 1 if kind == 'cell' else 2
    exact = float(scale) == 1.0 and float(D0) == np.rint(D0)
    D0i = int(np.rint(D0)) if exact else 0
    den = O[G][G] + D0i
    S1 = [n[g] * den - c * O[g][G] for g in range(G)]
    S2 = [[n[g] * n[k] * den - c * n[g] * O[k][G] - c * n[k] * O[g][G] + c * c * O[g][k] for k in range(G)] for g in range(G)]
    if exact:
        if den <= 0:
            raise ValueError('no pair of distinct samples carries weight')
        mean = np.array([v / den for v in S1], dtype=np.float64).reshape(G)
        return mean, np.array([[v / den for v in r] for r in S2], dtype=np.float64).reshape(G, G)
    s2 = float(scale) * float(scale)
    nf = np.array(n, dtype=np.float64)
    den = float(den) / s2 + float(D0)
    if not den > 0:
        raise ValueError('no pair of distinct samples carries weight')
    mean = (np.array([float(v) for v in S1], dtype=np.float64).reshape(G) / s2 + D0 * nf) / den
    return mean, (np.array([[float(v) for v in r] for r in S2], dtype=np.float64).reshape(G, G) / s2 + D0 * np.outer(nf, nf)) / den


def chi_of_k(QQ, N):
    """chi(k_m) = (1 / N) sum_{g,g'} <Q_g Q_g'> cos(k_m (g - g')), k_m = 2 pi m / G, m = 0 .. G // 2.  At k != 0 the G^2 terms cancel
    down to a small remainder, so they are added up without rounding (math.fsum): what error is left is that of the terms."""
    import math
    QQ = np.asarray(QQ, dtype=np.float64)
    G = QQ.shape[0]
    dg = np.arange(G)[:, None] - np.arange(G)[None, :]
    return np.array([math.fsum((QQ * np.cos(2.0 * np.pi * m * dg / G)).ravel()) for m in range(G // 2 + 1)], dtype=np.float64) / float(N)


def correlation_length(QQ, N):
    """(chi (G // 2 + 1,), xi): xi = 1 / (2 sin(pi / G)) sqrt(chi(0) / chi(k_1) - 1), the second-moment correlation length in units of
    lattice lines.  nan when G < 2 or the ratio is below 1; a chi(k_1) that is zero to rounding -- not above G^2 2^-52 sum |<Q Q'>| / N,
    the rounding error of its own sum -- has no ratio and gives nan as well."""
    QQ = np.asarray(QQ, dtype=np.float64)
    G = QQ.shape[0]
    chi = chi_of_k(QQ, N)
    if G < 2:
        return chi, float('nan')
    floor = G * G * 2.0 ** -52 * float(np.sum(np.abs(QQ))) / float(N)
    if not chi[1] > floor or not chi[0] / chi[1] >= 1.0:
        return chi, float('nan')
    return chi, float(np.sqrt(chi[0] / chi[1] - 1.0) / (2.0 * np.sin(np.pi / G)))


def _line_source(solver, kind):
    """(what is compared (M, n), lanes16)"""
    return (cell_states(solver).astype(np.int64), True) if kind == 'cell' else (spin_bits(solver), False)


def overlap_correlations(solver, axis='both', kind=None, weights='uniform'):
    """calculate_overlap_correlations of tnac4o (documented there)."""
    if axis not in ('x', 'y', 'both'):
        raise ValueError("axis must be 'x', 'y' or 'both'")
    if kind == 'link':
        raise ValueError("kind 'link' has no line-resolved overlap: a coupling lies in two groups")
    kind, w = check_arguments(solver, kind, weights)
    axes = ('x', 'y') if axis == 'both' else (axis,)
    lanes16 = kind == 'cell'
    per = 4 if lanes16 else 64
    plan = {}
    for ax in axes:                                                   # every refusal comes before any device work
        group, sizes = line_groups(solver, ax, kind)
        G, wpg = sizes.size, max(1, -(-int(sizes.max()) // per))
        if G > MAX_GROUPS:
            raise NotImplementedError("axis '%s' has %d lattice lines; tn_pair_moments takes at most %d groups (its distance table must fit "
                                      'the 160 KiB of LDS); there is no host fallback' % (ax, G, MAX_GROUPS))
        if wpg > MAX_GROUP_WORDS:
            raise NotImplementedError("kind '%s', axis '%s': a lattice line holds %d %s, %d words; tn_pair_moments takes at most %d words per "
                                      'group; there is no host fallback' % (kind, ax, int(sizes.max()), 'cells' if lanes16 else 'spins', wpg,
                                                                            MAX_GROUP_WORDS))
        if int(sizes.sum()) < 1:
            raise ValueError("kind '%s': the model has nothing to compare" % kind)
        plan[ax] = (group, sizes, G, wpg)
    from . import ops
    X, _ = _line_source(solver, kind)
    C, mean, chi, xi, xil, nsz = {}, {}, {}, {}, {}, {}
    for ax in axes:
        group, sizes, G, wpg = plan[ax]
        rows, wpg = pack_groups(X, group, G, lanes16)
        wmax = WMAX // (per * wpg)
        urows, wq, scale, D0 = prepare(rows, w, wmax)
        if urows.shape[0] >= 2:
            d_rows, d_w = upload(urows, wq)
            limbs = ops.pair_moments(d_rows, G, wpg, d_w, wmax, lanes16).cpu().numpy()
        else:                                        # one distinct row: every pair sits in D0
            limbs = np.zeros((G + 1, G + 1, 2), dtype=np.int64)
        Q1, QQ = second_moments(limbs, sizes, kind, scale, D0)
        nf = np.where(sizes > 0, sizes, 1).astype(np.float64)
        empty = sizes == 0
        mean[ax] = np.where(empty, np.nan, Q1 / nf)
        C[ax] = np.where(empty[:, None] | empty[None, :], np.nan, QQ / np.outer(nf, nf))
        chi[ax], xi[ax] = correlation_length(QQ, int(sizes.sum()))
        xil[ax] = xi[ax] / G
        nsz[ax] = sizes.copy()
    solver.overlap_line_kind = kind
    solver.overlap_line_correlations = C
    solver.overlap_line_mean = mean
    solver.overlap_line_sizes = nsz
    solver.overlap_chi = chi
    solver.overlap_xi = xi
    solver.overlap_xi_over_L = xil
    solver.overlap_ess = effective_sample_size(w)
    return C


# ---------------------------------------------------------------------------------------------- every pair of spins
MAX_SPIN_BITS = 65534            # largest row tn_spin_moments takes: nbits + 2 rows and columns, at most 2^16 (include/tnpeps.h)


def pair_weight(W, S2, scale=1.0):
    """(W, S2, W^2 - S2) in the arithmetic spin_estimators uses: W = sum_a w_a an integer, S2 = sum_a w_a^2 over the raw samples in units
    of scale^2.  scale 1 and an integer S2: np.int64 while W < 2^31 (the square fits), Python integers above; otherwise float64.
    W^2 - S2 = sum_{a != b} w_a w_b must be positive -- in float64 above 2^-40 W^2, what the rounding of the weights to 32 bits can
    leave of a single sample -- or: ValueError."""
    W = int(W)
    if float(scale) == 1.0 and float(S2) == np.rint(S2):
        Wn, S2n = (np.int64(W), np.int64(int(np.rint(S2)))) if W < 2 ** 31 else (W, int(np.rint(S2)))
        floor = 0
    else:
        Wn, S2n = float(W), float(S2)
        floor = 2.0 ** -40 * Wn * Wn
    den = Wn * Wn - S2n
    if not W > 0 or not den > floor:
        raise ValueError('no pair of distinct samples carries weight')
    return Wn, S2n, den


def spin_estimators(out, S2, scale=1.0):
    """(m (n,), C (n, n), QQ (n, n)) in float64 from the integers of tn_spin_moments: out (n+2, n+2) (any integer dtype, read as
    unsigned 64-bit; or nested Python integers), D_ij = out[i][j] the weight of the samples in which bits i and j differ,
    W = out[n][n+1] the total weight.  m_i = (W - 2 out[i][n+1]) / W = <sigma_i> with sigma = +1 where the bit is 1 (binary_states
    writes 1 there: the convention of `magnetization`), C_ij = (W - 2 D_ij) / W = <sigma_i sigma_j>, and the pair estimator over the
    distinct samples QQ_ij = <q_i q_j> = sum_{a != b} w_a w_b (s_i s_j)_a (s_i s_j)_b / sum_{a != b} w_a w_b
    = ((W - 2 D_ij)^2 - S2) / (W^2 - S2), S2 = sum_a w_a^2 over the raw samples in units of scale^2.  With scale 1 and an integer S2
    everything up to the final divisions is exact: in int64 while W < 2^31, in Python integers above.  With a scale the weights were
    rounded; the expression is then formed in float64, whose error (2^-52 of W^2, like the denominator) is far below the
    rounding of the weights (pair_weight).  Fewer than two samples with weight: ValueError."""
    O = np.asarray(out)
    if O.dtype != object:
        O = np.ascontiguousarray(O).astype(np.int64, copy=False).view(np.uint64)
    n = O.shape[0] - 2
    if O.ndim != 2 or O.shape != (n + 2, n + 2) or n < 1:
        raise ValueError('out (n+2, n+2) expected')
    W = int(O[n, n + 1])
    Wn, S2n, den = pair_weight(W, S2, scale)
    D = O.astype(np.int64 if isinstance(Wn, np.int64) else np.float64 if isinstance(Wn, float) else object)
    A = Wn - 2 * D[:n, :n]
    m = (Wn - 2 * D[:n, n + 1]).astype(np.float64) / float(W)
    C = A.astype(np.float64) / float(W)
    QQ = (A * A - S2n).astype(np.float64) / float(den)
    return m, C, QQ


def chi_sg_2d(QQ, gx, gy, Nx, Ny):
    """chi_SG(k_x, k_y) = (1 / N) sum_ij <q_i q_j> cos(k_x (x_i - x_j) + k_y (y_i - y_j)) on the grid k = 2 pi (m_x / Nx, m_y / Ny):
    (Nx, Ny) float64, entry [m_x, m_y].  gx, gy (n,): the model column and row of spin i's cell (line_groups).  <q_i q_j> is summed
    into blocks of cell pairs first; the (Nx Ny)^2 terms of a wave vector cancel at k != 0, so they are added without rounding
    (math.fsum, as chi_of_k).  The phase is reduced in integers, k.r = 2 pi ((m_x dx Ny + m_y dy Nx) mod Nx Ny) / (Nx Ny);
    chi(-k) = chi(k) is computed once."""
    import math
    QQ = np.asarray(QQ, dtype=np.float64)
    gx, gy = np.asarray(gx, dtype=np.int64), np.asarray(gy, dtype=np.int64)
    n, nc = QQ.shape[0], Nx * Ny
    cell = gy * Nx + gx
    Z = np.zeros((n, nc))
    Z[np.arange(n), cell] = 1.0
    B = Z.T @ QQ @ Z                                                    # blocks of cell pairs
    cx, cy = np.arange(nc) % Nx, np.arange(nc) // Nx
    dx, dy = cx[:, None] - cx[None, :], cy[:, None] - cy[None, :]
    table = np.cos(2.0 * np.pi * np.arange(nc) / nc)
    chi = np.zeros((Nx, Ny))
    for mx in range(Nx):
        for my in range(Ny):
            tx, ty = (-mx) % Nx, (-my) % Ny
            if (tx, ty) < (mx, my):
                chi[mx, my] = chi[tx, ty]
                continue
            phase = (mx * dx * Ny + my * dy * Nx) % nc
            chi[mx, my] = math.fsum((B * table[phase]).ravel()) / float(n)
    return chi


def sample_correlations(solver, weights='uniform'):
    """calculate_sample_correlations of tnac4o (documented there)."""
    _ising(solver, 'calculate_sample_correlations')
    _, w = check_arguments(solver, 'spin', weights)
    bits = spin_bits(solver)
    n = int(bits.shape[1])
    if n < 1:
        raise ValueError('the model has no active spin')
    if n > MAX_SPIN_BITS:
        raise NotImplementedError('the model has %d active spins; tn_spin_moments takes at most %d; there is no host fallback' % (n, MAX_SPIN_BITS))
    gx, gy = line_groups(solver, 'x', 'spin')[0], line_groups(solver, 'y', 'spin')[0]
    urows, wq, scale, _ = prepare(pack_bits(bits), w)
    S2 = float(np.sum(w * w)) * scale * scale
    pair_weight(int(wq.astype(np.uint64).sum(dtype=object)) if wq.size else 0, S2, scale)   # every refusal comes before any device work
    from . import ops
    d_rows, d_w = upload(urows, wq)
    out = ops.spin_moments(d_rows, n, d_w, int(wq.max())).cpu().numpy()
    m, C, QQ = spin_estimators(out, S2, scale)
    chi = chi_sg_2d(QQ, gx, gy, int(solver.Nx_model), int(solver.Ny_model))
    solver.sample_spins = active_spins(solver)
    solver.sample_magnetization = m
    solver.sample_correlations = C
    solver.sample_overlap_correlations = QQ
    solver.sample_chi_sg = chi
    solver.overlap_ess = effective_sample_size(w)
    return C
