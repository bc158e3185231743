"""References, error bounds and seeded cases for the direct tests of the beam-side kernels (no GPU, no torch): tn_calc_pn and its
twins tn_sample_pn / tn_score_pn (the table of csrc/pn.h), tn_env_rr_batched, tn_env_rl_batched, tn_merge_groups, tn_nfactor_batched.
tests/test_beam_kernels_host.py checks the references and the cases on the CPU; tests/test_gpu_beam_kernels.py runs the kernels.

- pn_table_ref: the conditional table of one branch (reference tnac4o.py:1792-1807) in mpmath at 40 digits, with a running error
  bound per entry that follows from the kernel's arithmetic (u = 2^-53):
      raw entry     e_s   = (Dr + 1) u |F_s| sum_c |t1[d, c]| |rr[c, r]|        (sequential dot of length Dr, one product)
      lifted entry  e_s   = e_min                                                  (it is a copy of |min|)
      total         E     = sum e_s + (ceil(q / 256) + 8) u sum |sP|              (per-thread strided sums, then a 256-leaf tree)
      table         tol_s = (e_s + |P_s| E) / no + 3 u |P_s|
      flag          tol   = |minP| (e_min / |min| + E / no + 3 u)
  The GPU test asserts 2 x tol; pn_table_emul (float64, the kernel's order of operations) stays within 1 x tol on the CPU.
  `ambiguous` counts the entries whose comparison with |min| could come out the other way within the bounds (and a second smallest
  entry, or a zero, within bounds of the minimum): the cases are chosen so that it is 0 -- a condition on the inputs, not a tolerance.
- log2p_ref: correctly rounded log2 of a table plus a parent log-probability.
- env_rr_ref: the two contractions of tnac4o.py:1779-1781 evaluated EXACTLY (every double is an integer times a power of two; Python
  integers), which at chi = 128 takes a second where 40-digit mpmath takes minutes; bound (Dr + br + 2) u sum |A| |RR| |W| per element
  (one accumulator runs over all p Dr terms, so a strict worst case would carry p Dr + br; rounding errors do not line up that way, and
  the sum of magnitudes is far above the result on data with signs: the device stays below 0.5 x the bound).
- merge_groups_ref, env_rl_ref, nfactor_batched_ref: float64 in the kernels' stated order, comparable bit for bit.
- PN_CASES / pn_case, ENV_RR_CASES / env_rr_case, MERGE_CASES / merge_case, env_rl_case, nfactor_block: the seeded inputs."""
import functools
import math
from types import SimpleNamespace

import numpy as np

from oracle import mps_ref

U = 2.0 ** -53
DPS = 40
LDS_LIMIT = 150 * 1024
NEG_INF = -math.inf


def pn_front_doubles(p, Dr, br):
    return p * Dr + Dr * br + p * br


def calc_pn_lds(q, p, Dr, br):
    """Dynamic LDS of tn_calc_pn and tn_score_pn, bytes."""
    return (pn_front_doubles(p, Dr, br) + q) * 8


def sample_pn_lds(q, p, Dr, br):
    """Dynamic LDS of tn_sample_pn (the table and its running sum), bytes."""
    return (max(pn_front_doubles(p, Dr, br), q) + q) * 8


def env_rr_lds(p, Dr, bl, br):
    return (Dr * br + bl * p * br + Dr * bl) * 8


def hi_lo(x_mp):
    """A high-precision number as float64 head and tail."""
    hi = float(x_mp)
    return hi, float(x_mp - hi)


# ------------------------------------------------------------------------------------------------------------ the table of pn.h
@functools.lru_cache(maxsize=64)
def _t2_cached(p, Dr, br, t1_bytes, rr_bytes):
    import mpmath
    t1 = np.frombuffer(t1_bytes, dtype=np.float64).reshape(p, Dr)
    rr = np.frombuffer(rr_bytes, dtype=np.float64).reshape(Dr, br)
    with mpmath.workdps(DPS):
        rows = [[mpmath.mpf(float(x)) for x in t1[d]] for d in range(p)]
        cols = [[mpmath.mpf(float(x)) for x in rr[:, r]] for r in range(br)]
        T2 = [[mpmath.fdot(rows[d], cols[r]) for r in range(br)] for d in range(p)]
    return T2, np.abs(t1) @ np.abs(rr)


def pn_table_ref(t1, rr, F, dmap, rmap, l, u, exact=False):
    """Table of the branch (t1 (p, Dr), rr (Dr, br), F[:, l, u]) at 40 digits.  exact=True: the inputs are small integers on which every
    operation of the kernel up to the normalisation is exact, so only the 3 u |P| of the normalisation remains.
    Returns P / P_lo (head and tail), minP / minP_lo, count (lifted entries), tol (per entry), tol_min, ambiguous, raw (float64 of the
    entries before the rule), no (their sum after the rule)."""
    import mpmath
    t1 = np.ascontiguousarray(t1, dtype=np.float64)
    rr = np.ascontiguousarray(rr, dtype=np.float64)
    p, Dr = t1.shape
    br = rr.shape[1]
    f = np.asarray(F, dtype=np.float64)[:, l, u]
    q = f.size
    dm, rm = np.asarray(dmap).astype(np.int64), np.asarray(rmap).astype(np.int64)
    T2, T2abs = _t2_cached(p, Dr, br, t1.tobytes(), rr.tobytes())
    idx = np.arange(q)
    with mpmath.workdps(DPS):
        raw = [mpmath.mpf(float(f[s])) * T2[dm[s]][rm[s]] for s in range(q)]
        e = np.zeros(q) if exact else (Dr + 1) * U * np.abs(f) * T2abs[dm, rm] * (1.0 + 2.0 ** -30)
        rawf = np.array([float(x) for x in raw])
        imin = min(range(q), key=raw.__getitem__)
        m, e_min = raw[imin], float(e[imin])
        sP, es, amb, count = list(raw), e.copy(), 0, 0
        if m < 0:
            a = -m
            lifted = np.array([x < a for x in raw])
            count = int(lifted.sum())
            for s in np.flatnonzero(lifted):
                sP[s] = a
            es[lifted] = e_min
            gap = np.array([float(abs(x - a)) for x in raw])
            width = e + e_min
            amb += int(np.sum((width > 0) & (gap <= width) & (idx != imin)))
            if q > 1:                                            # a second smallest entry within bounds of the minimum
                d2 = np.array([float(x - m) for x in raw])
                amb += int(np.any((idx != imin) & (width > 0) & (d2 <= width)))
            amb += int(e_min > 0 and float(a) <= e_min)          # the sign of the minimum itself
        else:
            amb += int(np.sum((e > 0) & (rawf - e < 0)))         # an entry that could come out negative
        no = mpmath.fsum(sP)
        E = 0.0 if exact else float(np.sum(es)) + (math.ceil(q / 256) + 8) * U * float(mpmath.fsum([abs(x) for x in sP]))
        if no > 0:
            nof = float(no)
            amb += int(nof <= E)
            Pm = [x / no for x in sP]
            mP = (m * count if m < 0 else m) / no
            P = np.array([float(x) for x in Pm])
            P_lo = np.array([float(x - h) for x, h in zip(Pm, P)])
            tol = (es + np.abs(P) * E) / nof + 3 * U * np.abs(P)
            minP, minP_lo = hi_lo(mP)
            tol_min = (max(count, 1) * e_min + abs(minP) * E) / nof + 3 * U * abs(minP)
        else:                                                    # all zeros: exactly uniform, flag exactly -1
            nof = 0.0
            P, P_lo, tol = np.full(q, 1.0 / q), np.zeros(q), np.zeros(q)
            minP, minP_lo, tol_min = -1.0, 0.0, 0.0
    return SimpleNamespace(P=P, P_lo=P_lo, minP=minP, minP_lo=minP_lo, count=count, tol=tol, tol_min=tol_min, ambiguous=amb, raw=rawf,
                           no=nof, q=q)


def _ratio(err, tol):
    """max err / tol, where a zero tolerance asks for equality."""
    err, tol = np.atleast_1d(np.asarray(err, dtype=np.float64)), np.atleast_1d(np.asarray(tol, dtype=np.float64))
    out = np.zeros(err.shape)
    z = tol == 0
    out[z] = np.where(err[z] == 0, 0.0, np.inf)
    out[~z] = err[~z] / tol[~z]
    out[np.isnan(err)] = np.inf
    return float(out.max())


def pn_error_ratios(ref, P, minP):
    """(worst |P - ref| / tol over the table, |minP - ref| / tol_min) of a float64 table against pn_table_ref's."""
    P = np.asarray(P, dtype=np.float64)
    return (_ratio(np.abs((P - ref.P) - ref.P_lo), ref.tol), _ratio(abs((float(minP) - ref.minP) - ref.minP_lo), ref.tol_min))


def regime_of(ref):
    """'zero' | 'positive' | 'partial' (0 < count < q, -1 < minP < 0) | 'dominated' (everything lifted) | 'other'."""
    if ref.no == 0:
        return 'zero'
    if ref.count == 0:
        return 'positive' if ref.raw.min() >= 0 and ref.minP >= 0 else 'other'
    if ref.count == ref.q:
        return 'dominated'
    return 'partial' if -1.0 < ref.minP < 0.0 else 'other'


def block_sum_emul(x):
    """Sum of x as pn_table forms it: thread t adds x[t], x[t + 256], ... in order, then a binary tree over the 256 partial sums."""
    x = np.asarray(x, dtype=np.float64)
    pad = np.zeros(-(-x.size // 256) * 256)
    pad[:x.size] = x
    part = np.zeros(256)
    for row in pad.reshape(-1, 256):
        part = part + row
    k = 128
    while k:
        part[:k] = part[:k] + part[k:2 * k]
        k //= 2
    return float(part[0])


def pn_table_emul(t1, rr, F, dmap, rmap, l, u):
    """pn_table of csrc/pn.h in float64 numpy, operation by operation (the device may fuse a multiply into an add, so this is an
    instance of the arithmetic the bound covers, not a bit-for-bit twin).  Returns (P, minP)."""
    t1, rr = np.asarray(t1, dtype=np.float64), np.asarray(rr, dtype=np.float64)
    T2 = np.zeros((t1.shape[0], rr.shape[1]))
    for c in range(t1.shape[1]):
        T2 = T2 + t1[:, c:c + 1] * rr[c:c + 1, :]
    sP = np.asarray(F, dtype=np.float64)[:, l, u] * T2[np.asarray(dmap), np.asarray(rmap)]
    q = sP.size
    m = float(sP.min())
    if m < 0:
        low = sP < abs(m)
        sP = np.where(low, abs(m), sP)
        m = m * float(low.sum())
    no = block_sum_emul(sP)
    if no > 0:
        inv = 1.0 / no
        return sP * inv, m * inv
    return sP + 1.0 / q, -1.0


def log2p_ref(P_dev, base):
    """Correctly rounded log2(P) + base per entry (mpmath, 40 digits): -inf where P == 0 or base == -inf."""
    import mpmath
    P = np.asarray(P_dev, dtype=np.float64).reshape(-1)
    out = np.empty(P.size)
    with mpmath.workdps(DPS):
        b = None if base == NEG_INF else mpmath.mpf(float(base))
        for i, x in enumerate(P):
            out[i] = NEG_INF if (x == 0 or b is None) else float(mpmath.log(mpmath.mpf(float(x)), 2) + b)
    return out


def ulps(got, ref):
    """|got - ref| in units of the spacing of ref (finite entries)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.abs(got - ref) / np.spacing(np.abs(ref))


# ---- the cases of the table
PN_SITE = (16, 64, 16)                                           # p, Dr, br of the workload's bulk cell at chi = 64


def _branches(q, nl, nu):
    """(pref, suf, l, u, regime): prefix 0 positive, 1 with a slightly negative row, 2 (the last) with a dominating negative row; suffix 1
    zero, 0 and 2 (the last) positive.  Branches share prefixes and suffixes, differ in l alone and in u alone, and use the last l / u."""
    L, Up = nl - 1, nu - 1
    if q == 1:
        return [(0, 0, 0, 0, 'positive'), (1, 0, 0, 0, 'dominated'), (0, 1, 0, 0, 'zero'), (2, 2, 0, 0, 'dominated')]
    out = [(0, 0, 0, 0, 'positive')]
    if nl > 1:
        out.append((0, 0, L, 0, 'positive'))
    if nu > 1:
        out.append((0, 0, 0, Up, 'positive'))
    out += [(1, 2, L, Up, 'partial'), (1, 0, 0, 0, 'partial'), (2, 2, L // 2, Up // 2, 'dominated'), (0, 1, 0, 0, 'zero'), (0, 2, L, Up, 'positive')]
    return out


_BIG = [(0, 0, 0, 0, 'positive'), (1, 2, 0, 0, 'partial'), (2, 2, 0, 0, 'dominated'), (0, 1, 0, 0, 'zero')]

# name -> (shape (q, p, Dr, br, nl, nu), seed); the seeds are the first tried unless a comment says otherwise
PN_CASES = {
    'smallest': ((1, 1, 1, 1, 1, 1), 1),
    'nl_ne_nu': ((3, 2, 1, 3, 2, 1), 2),
    'stride255': ((255, 6, 7, 5, 3, 2), 3),
    'stride256': ((256, 6, 7, 5, 3, 2), 4),
    'stride257': ((257, 6, 7, 5, 3, 2), 5),
    'long_dot': ((513, 3, 200, 2, 1, 4), 6),
    'workload': ((256, 16, 64, 16, 16, 16), 7),
    'chi128': ((256, 16, 128, 16, 16, 16), 8),
    'lds48k_below': ((3840,) + PN_SITE + (1, 1), 9),
    'lds48k_above': ((3841,) + PN_SITE + (1, 1), 10),
    'lds64k_below': ((5888,) + PN_SITE + (1, 1), 11),
    'lds64k_above': ((5889,) + PN_SITE + (1, 1), 12),
    'lds150k_limit': ((16896,) + PN_SITE + (1, 1), 13),
    'sample48k_below': ((3072,) + PN_SITE + (1, 1), 14),      # tn_sample_pn keeps the running sum too: (max(front, q) + q) * 8
    'sample48k_above': ((3073,) + PN_SITE + (1, 1), 15),
    'sample150k_limit': ((9600,) + PN_SITE + (1, 1), 16),
    'exact12': ((12, 2, 2, 2, 1, 1), 0),
    'exact384': ((384, 2, 2, 2, 1, 1), 0),
}
PN_REFUSED = {'refused_calc': ((16897,) + PN_SITE + (1, 1), 17), 'refused_sample': ((9601,) + PN_SITE + (1, 1), 18)}      # 8 / 16 bytes too many
EXACT_RAW = (-2, 2, 2, 2, 1, 0, -1, 2, 4, 4, 4, 4)               # after the rule: 8 x 2 + 4 x 4 = 32; 4 entries lifted; 4 equal to |min|
_EXACT_FDR = {-2: (2, 0, 1), 2: (1, 1, 0), 1: (1, 0, 0), 0: (0, 1, 1), -1: (1, 0, 1), 4: (2, 1, 0)}     # raw = F * T2[d, r], T2 = [[1, -1], [2, 1]]


@functools.lru_cache(maxsize=None)
def pn_case(name):
    """Inputs of a case: T1 (3, p, Dr), RR (3, Dr, br), F (q, nl, nu), dmap, rmap (int32), branches (nb, 4) int32 = pref, suf, l, u,
    regimes (per branch), base (parent log-probabilities, one of them -inf), exact."""
    (q, p, Dr, br, nl, nu), seed = PN_CASES[name] if name in PN_CASES else PN_REFUSED[name]
    if name.startswith('exact'):
        T1 = np.array([[[1.0, 0.0], [1.0, 1.0]]])
        RR = np.array([[[1.0, -1.0], [1.0, 2.0]]])
        pat = [_EXACT_FDR[v] for v in EXACT_RAW] * (q // 12)
        F = np.array([x[0] for x in pat], dtype=np.float64).reshape(q, 1, 1)
        dmap, rmap = np.array([x[1] for x in pat], dtype=np.int32), np.array([x[2] for x in pat], dtype=np.int32)
        return SimpleNamespace(name=name, shape=(q, p, Dr, br, nl, nu), T1=T1, RR=RR, F=F, dmap=dmap, rmap=rmap,
                               branches=np.zeros((1, 4), dtype=np.int32), regimes=['partial'], base=np.array([0.0]), exact=True)
    rng = np.random.default_rng([77, seed])
    T1 = rng.uniform(0.1, 1.0, (3, p, Dr))
    T1[1, 0] *= -0.01
    T1[2, 0] *= -1000.0
    RR = rng.uniform(0.1, 1.0, (3, Dr, br))
    RR[1] = 0.0
    F = rng.uniform(0.1, 1.0, (q, nl, nu))
    if q >= 8:
        F[rng.random((q, nl, nu)) < 0.2] = 0.0                  # zero entries: log2 gives -inf there
    F[0] = rng.uniform(0.5, 1.0, (nl, nu))
    dmap, rmap = rng.integers(0, p, q).astype(np.int32), rng.integers(0, br, q).astype(np.int32)
    dmap[0] = 0
    if q > 1:
        dmap[q - 1], rmap[q - 1] = p - 1, br - 1
        F[q - 1] = rng.uniform(0.5, 1.0, (nl, nu))
    br_list = _BIG if q > 1024 else _branches(q, nl, nu)
    branches = np.array([b[:4] for b in br_list], dtype=np.int32)
    base = -(0.3 + 3.7 * np.arange(len(br_list)))
    base[0] = 0.0
    base[1] = NEG_INF
    return SimpleNamespace(name=name, shape=(q, p, Dr, br, nl, nu), T1=T1, RR=RR, F=F, dmap=dmap, rmap=rmap, branches=branches,
                           regimes=[b[4] for b in br_list], base=base, exact=False)


@functools.lru_cache(maxsize=None)
def pn_case_refs(name):
    """pn_table_ref of every branch of the case (computed once per process)."""
    c = pn_case(name)
    return [pn_table_ref(c.T1[b[0]], c.RR[b[1]], c.F, c.dmap, c.rmap, int(b[2]), int(b[3]), exact=c.exact) for b in c.branches]


# ------------------------------------------------------------------------------------------------------------ tn_env_rr_batched
def _to_int(a):
    """a (float64) == ints * 2**e exactly: (object array of Python integers, e)."""
    a = np.asarray(a, dtype=np.float64)
    out = np.zeros(a.shape, dtype=object)
    nz = a != 0
    if not nz.any():
        return out, 0
    mant, ex = np.frexp(a)
    e = int(ex[nz].min()) - 53
    mi = (mant * 2.0 ** 53).astype(np.int64)
    of, mf, xf = out.reshape(-1), mi.reshape(-1), ex.reshape(-1)
    for i in np.flatnonzero(nz.reshape(-1)):
        of[i] = int(mf[i]) << (int(xf[i]) - 53 - e)
    return out, e


def _int_hi_lo(n, e):
    """The integer n times 2**e as float64 head and tail."""
    hi = float(n)
    lo = float(n - int(hi))
    return math.ldexp(hi, e), math.ldexp(lo, e)


def env_rr_exact(A, RR, Wu):
    """out[x, l] = sum_{d, x', r} A[x, d, x'] RR[x', r] Wu[l, d, r] without rounding: (object array of integers (Dl, bl), exponent)."""
    Dl, p, Dr = A.shape
    bl = Wu.shape[0]
    Ai, ea = _to_int(A)
    Ri, er = _to_int(RR)
    Wi, ew = _to_int(Wu)
    V = np.concatenate([np.dot(Ri, Wi[:, d, :].T) for d in range(p)], axis=0)      # (p Dr, bl): V_d = RR . W_d^T
    return np.dot(Ai.reshape(Dl, p * Dr), V), ea + er + ew


def env_rr_ref(A, RR, Wu):
    """One key of tn_env_rr_batched before its normalisation.  Returns hi / lo (head and tail of the exact block), bound per element,
    expo (floor(log2 max|block|); None for a zero block) and ambiguous (the largest magnitude lies within the bounds of a power of two,
    so the normalisation could come out as another one)."""
    A, RR, Wu = (np.asarray(x, dtype=np.float64) for x in (A, RR, Wu))
    Dl, p, Dr = A.shape
    bl, _, br = Wu.shape
    absV = np.concatenate([np.abs(RR) @ np.abs(Wu[:, d, :]).T for d in range(p)], axis=0)
    bound = (Dr + br + 2) * U * (np.abs(A).reshape(Dl, p * Dr) @ absV) * (1.0 + 2.0 ** -30)
    if not RR.any() or not A.any() or not Wu.any():
        z = np.zeros((Dl, bl))
        return SimpleNamespace(hi=z, lo=z.copy(), bound=z.copy(), expo=None, ambiguous=0)
    ints, e = env_rr_exact(A, RR, Wu)
    hl = np.array([_int_hi_lo(int(n), e) for n in ints.reshape(-1)])
    hi, lo = hl[:, 0].reshape(Dl, bl), hl[:, 1].reshape(Dl, bl)
    mag = np.abs(hi)
    M = float(mag.max())
    if M == 0.0:
        return SimpleNamespace(hi=hi, lo=lo, bound=bound, expo=None, ambiguous=0)
    expo = math.frexp(M)[1] - 1
    low, high = math.ldexp(1.0, expo), math.ldexp(1.0, expo + 1)
    amb = int(np.any(mag + bound >= high) or float((mag - bound).max()) < low)
    return SimpleNamespace(hi=hi, lo=lo, bound=bound, expo=expo, ambiguous=amb)


def env_rr_error_ratio(ref, out):
    """Worst |out * 2^expo - exact| / bound of a returned (normalised) block; a zero block must come back as zeros."""
    out = np.asarray(out, dtype=np.float64)
    if ref.expo is None:
        return 0.0 if not out.any() else math.inf
    return _ratio(np.abs((np.ldexp(out, ref.expo) - ref.hi) - ref.lo), ref.bound)


# name -> (Dl, p, Dr, bl, br, pu), seed
ENV_RR_CASES = {
    'chi128': ((128, 16, 128, 16, 16, 16), 1),                   # 2048 outputs (all 8 accumulator slots), 64 KiB of LDS
    'partial_slot': ((113, 16, 64, 16, 16, 3), 2),               # 1808 outputs: the last slot partly used
    'slot5': ((65, 4, 9, 16, 3, 2), 3),                          # 1040 outputs
    'lds96k': ((128, 32, 128, 16, 16, 2), 4),
    'lds150k_limit': ((3, 74, 2, 16, 16, 2), 5),                 # (32 + 256 p + 32) * 8 <= 150 KiB  <=>  p <= 74
}
ENV_RR_REFUSED = {'refused_lds': ((3, 75, 2, 16, 16, 2), 6), 'refused_accumulators': ((2049, 1, 1, 1, 1, 1), 7)}


@functools.lru_cache(maxsize=None)
def env_rr_case(name):
    """A, RRprev (3 parents; parent 1 all zero), W, parent, uidx (3 keys: the zero parent, the first and the last parent / up index):
    graded data as tests/test_gpu_kernels.py::test_env_rr_batched."""
    (Dl, p, Dr, bl, br, pu), seed = ENV_RR_CASES[name] if name in ENV_RR_CASES else ENV_RR_REFUSED[name]
    rng = np.random.default_rng([78, seed])
    A = rng.standard_normal((Dl, p, Dr))
    RRp = rng.standard_normal((3, Dr, br)) * np.exp(-40 * rng.uniform(0, 1, (3, 1, 1)))
    RRp[1] = 0.0
    W = np.exp(-20 * rng.uniform(0, 1, (bl, p, br, pu)))
    parent = np.array([1, 0, 2], dtype=np.int32)
    uidx = np.array([0, 0, pu - 1], dtype=np.int32)
    return SimpleNamespace(name=name, shape=(Dl, p, Dr, bl, br, pu), A=A, RRp=RRp, W=W, parent=parent, uidx=uidx)


@functools.lru_cache(maxsize=None)
def env_rr_case_refs(name):
    c = env_rr_case(name)
    return [env_rr_ref(c.A, c.RRp[c.parent[k]], c.W[:, :, :, c.uidx[k]]) for k in range(c.parent.size)]


# ------------------------------------------------------------------------------------------------------------ bit-for-bit kernels
def env_rl_ref(T1, par, didx):
    """out[k] = T1[par[k], didx[k]] / nfactor of that row (a multiplication by the inverse power of two, as the kernel's)."""
    out = np.empty((len(par), T1.shape[2]))
    for k in range(len(par)):
        row = T1[par[k], didx[k]]
        out[k] = row * (1.0 / mps_ref.pow2_floor_max(row))
    return out


def nfactor_batched_ref(X):
    """Every block X[b] times the inverse of its own nfactor (2^-1023 for a zero or subnormal block: the factor 2^1023)."""
    return np.stack([x * (1.0 / mps_ref.pow2_floor_max(x)) for x in X])


def merge_groups_ref(E, lp, deg, pos, starts, min_dEng):
    """tn_merge_groups in its stated order: per group the position of the FIRST member of minimal energy, the sum of the degeneracies of
    the members with E - Emin <= min_dEng, and the representative's log2p when that set has one member, else the mean added up in
    member order.  An empty group gives (-1, 0, -inf).  Returns (rep_pos (int64), deg (int64), log2p (float64))."""
    ng = len(starts) - 1
    rep, dn, ln = np.empty(ng, dtype=np.int64), np.empty(ng, dtype=np.int64), np.empty(ng, dtype=np.float64)
    El, ll, dl = [float(x) for x in E], [float(x) for x in lp], [int(x) for x in deg]
    for g in range(ng):
        lo, hi = int(starts[g]), int(starts[g + 1])
        if lo >= hi:
            rep[g], dn[g], ln[g] = -1, 0, NEG_INF
            continue
        emin, first = El[lo], lo
        for i in range(lo + 1, hi):
            if El[i] < emin:
                emin, first = El[i], i
        cnt, d, acc = 0, 0, 0.0
        for i in range(lo, hi):
            if El[i] - emin <= min_dEng:
                cnt, d, acc = cnt + 1, d + dl[i], acc + ll[i]
        assert d < 2 ** 63
        rep[g], dn[g], ln[g] = pos[first], d, (acc / cnt if cnt > 1 else ll[first])
    return rep, dn, ln


MERGE_CASES = ('ng1', 'ng255', 'ng256', 'ng257', 'ng70001', 'generic', 'window_zero', 'window_edge', 'empty_only', 'empty_mixed', 'empty_many')
MERGE_EMPTY = ('empty_only', 'empty_mixed', 'empty_many')


def _merge_pack(groups, min_dEng, rng):
    """groups: list of (E, lp, deg) lists."""
    sizes = [len(g[0]) for g in groups]
    cat = lambda j, dt: np.array([x for g in groups for x in g[j]], dtype=dt)      # noqa: E731
    n = int(np.sum(sizes))
    return SimpleNamespace(E=cat(0, np.float64), lp=cat(1, np.float64), deg=cat(2, np.int64), pos=(rng.permutation(n) * 3 + 7).astype(np.int64),
                           starts=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), min_dEng=float(min_dEng), ng=len(groups))


def _merge_random(sizes, levels, step, min_dEng, rng):
    n = int(np.sum(sizes))
    return SimpleNamespace(E=rng.integers(0, levels, n) * step - 3.0, lp=-rng.uniform(0.0, 60.0, n), deg=rng.integers(1, 1000, n).astype(np.int64),
                           pos=(rng.permutation(n) * 3 + 7).astype(np.int64), starts=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                           min_dEng=float(min_dEng), ng=len(sizes))


@functools.lru_cache(maxsize=None)
def merge_case(name):
    """E, lp, deg, pos (exactly as long as the members), starts, min_dEng, ng.  Energies on a grid of exactly representable numbers, so
    that ties and members exactly at Emin + min_dEng occur and E - Emin is exact."""
    rng = np.random.default_rng([79, MERGE_CASES.index(name)])
    if name in ('ng1', 'ng255', 'ng256', 'ng257'):
        ng = int(name[2:])
        sizes = rng.integers(1, 1001, ng)
        sizes[0] = 1000
        sizes[-1] = 1 if ng > 1 else 1000
        return _merge_random(sizes, 4, 0.25, 0.25, rng)
    if name == 'ng70001':
        return _merge_random(rng.integers(1, 4, 70001), 3, 0.5, 0.0, rng)
    if name == 'generic':                                         # the reference's default window on energies that are not on a grid
        c = _merge_random(rng.integers(1, 40, 300), 4, 0.25, 1e-12, rng)
        c.E = rng.standard_normal(c.E.size)
        c.E[1::3] = c.E[0:-1:3][:c.E[1::3].size]                  # exact copies: ties inside and across groups
        return c
    i61 = 2 ** 61
    up = float(np.nextafter(1.25, 2.0))
    special = [([1.0], [-0.0], [3]),                                                          # alone: its own log2p, -0.0 kept
               ([2.0, 1.0, 1.0, 3.0, 1.0], [-1.0, -2.0, -5.0, -7.0, -11.0], [1, 2, 3, 4, 5]),   # ties: the first of the minima
               ([1.0, 1.25, up, 1.0], [-3.0, -4.0, -100.0, -6.5], [7, 11, 13, 17]),            # exactly at the edge, and one ulp past it
               ([5.0, 4.0, 9.0], [-1.0, -0.0, -2.0], [1, 1, 1]),                                # the representative alone among several
               ([1.0, 1.0, 1.0], [-3.0, NEG_INF, -4.0], [1, 2, 3]),                             # a -inf member in the set
               ([1.0, 7.0, 1.0], [-3.0, NEG_INF, -4.0], [1, 2, 3]),                             # a -inf member outside it
               ([2.0, 8.0], [NEG_INF, -1.0], [4, 4]),                                           # a -inf representative, alone
               ([0.0, 0.0, 0.0, 0.0], [-1.0, -2.0, -3.0, -4.0], [i61, i61, 2 ** 60, 5])]        # degeneracies adding up past 2^62
    if name == 'window_zero':
        return _merge_pack(special, 0.0, rng)
    if name == 'window_edge':
        return _merge_pack(special, 0.25, rng)
    if name == 'empty_only':
        return _merge_pack([([], [], [])], 0.25, rng)
    if name == 'empty_mixed':                                     # empty groups in the middle and at the end
        e = ([], [], [])
        return _merge_pack([special[1], e, special[2], e, e, special[0], e], 0.25, rng)
    sizes = rng.integers(0, 3, 600)                               # 'empty_many': three blocks of groups, a third of them empty
    sizes[[0, 255, 256, 599]] = 0
    return _merge_random(sizes, 4, 0.25, 0.25, rng)


ENV_RL_DR = (1, 63, 64, 65, 200)
ENV_RL_NK = (1, 4, 5, 50)


def env_rl_case(Dr, nk, first):
    """T1 (4, 3, Dr) graded by rows, with a zero row (1, 1), a subnormal row (2, 0) and the last row (3, 2); nk keys that start at the
    special row number `first` (0, 1, 2) and go round the three, then random rows."""
    rng = np.random.default_rng([80, Dr, nk, first])
    T1 = rng.standard_normal((4, 3, Dr)) * np.exp(-60 * rng.uniform(0, 1, (4, 3, 1)))
    T1[1, 1] = 0.0
    T1[2, 0] = rng.integers(1, 2 ** 40, Dr) * 5e-324
    special = [(1, 1), (2, 0), (3, 2)]
    keys = [special[(first + k) % 3] for k in range(min(nk, 3))] + [(int(rng.integers(0, 4)), int(rng.integers(0, 3))) for _ in range(max(nk - 3, 0))]
    return T1, np.array([k[0] for k in keys], dtype=np.int32), np.array([k[1] for k in keys], dtype=np.int32)


NFACTOR_LEN = (1, 255, 256, 257, 70000)
NFACTOR_KINDS = ('zero', 'subnormal', 'graded')


def nfactor_block(kind, n, seed):
    rng = np.random.default_rng([81, n, seed])
    if kind == 'zero':
        return np.zeros(n)
    if kind == 'subnormal':
        return rng.integers(-2 ** 40, 2 ** 40, n) * 5e-324 + 5e-324
    x = rng.standard_normal(n) * np.exp(-60 * rng.uniform(0, 1, n))
    x[int(rng.integers(0, n))] *= 2.0 ** int(rng.integers(-200, 200))          # the largest entry anywhere in the block
    return x
