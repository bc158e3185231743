"""Host references for the composed site and environment steps of the library (numpy only, no GPU).

Each function restates the DEFINING formula of one step -- the header comments of csrc/site.hip and csrc/marginal.hip and the
entry-point comments of include/tnpeps.h -- in np.longdouble, as a chain of pairwise einsum / tensordot calls, and returns the
result together with `absref`: the same contraction applied to the absolute values of the operands, the quantity every
rounding bound of a chain of products is relative to.

Bounds (u = 2^-53).  A chain of products with inner dimensions K_1 .. K_n evaluated in fp64 in ANY summation order (split-K,
the 4-deep MFMA step, FMA or not) obeys, element by element,
    |got - ref| <= gamma(K_1, .., K_n) * absref,      gamma = m u / (1 - m u),   m = sum K_i + n
(Higham, Accuracy and Stability of Numerical Algorithms, sections 3.1 and 3.5).  The longdouble reference's own error is
2^-11 of that and is ignored.  Normalised tables p_s / sum p with per-entry raw bounds delta_s = gamma * absraw_s:
    |dP_s| <= (delta_s + P_s sum(delta)) / sum_lifted,     |dlog2z| <= (sum(delta) / raw) / ln 2 + 4 u |log2z|.
"""
import numpy as np

import marginals_ref as mr

LD = np.longdouble
U = 2.0 ** -53


def gamma(*Ks):
    """gamma_m of a chain of products with the inner dimensions Ks: m = sum K_i + n."""
    m = int(sum(int(k) for k in Ks)) + len(Ks)
    return m * U / (1.0 - m * U)


def _ld(x):
    return np.asarray(x, dtype=LD)


def _with_abs(fn, *ops):
    """(fn(operands), fn(|operands|)), both in longdouble; a tuple-valued fn gives a tuple of such pairs."""
    a = fn(*[_ld(o) for o in ops])
    b = fn(*[np.abs(_ld(o)) for o in ops])
    if isinstance(a, tuple):
        return tuple(zip(a, b))
    return a, b


# ---------------------------------------------------------------------------------------------- csrc/site.hip
def rar(RL, A, RR):
    """out (c, s, c2) = RL (c x a) . A (a, s, a2) . RR (a2 x c2).  Chain: K = (a, a2)."""
    def f(RL, A, RR):
        T = np.tensordot(RL, A, axes=(1, 0))                       # (c, s, a2)
        return np.tensordot(T, RR, axes=(2, 0))                    # (c, s, c2)
    return _with_abs(f, RL, A, RR)


def env_mix(side, R, A, Ac):
    """side 0: out (c2 x a2) = sum_{c,s,a} Ac[c,s,c2] R[c,a] A[a,s,a2], R (c x a).  Chain: K = (a, c s).
    side 1: out (a x c) = sum_{s,a2,c2} A[a,s,a2] R[a2,c2] Ac[c,s,c2], R (a2 x c2).  Chain: K = (a2, s c2)."""
    def f0(R, A, Ac):
        T = np.tensordot(R, A, axes=(1, 0))                        # (c, s, a2)
        return np.tensordot(Ac, T, axes=((0, 1), (0, 1)))          # (c2, a2)

    def f1(R, A, Ac):
        T = np.tensordot(A, R, axes=(2, 0))                        # (a, s, c2)
        return np.tensordot(T, Ac, axes=((1, 2), (1, 2)))          # (a, c)
    return _with_abs(f0 if side == 0 else f1, R, A, Ac)


def apply_truncation(Al, U_, S, Vt, Ar):
    """Al (Dl, p, k0), U (k0 x keep), Vt (keep x k1), Ar (k1, p2, Dr), S (keep):
    ((Al.U, abs), (Vt.Ar, abs), diag(S)); diag(S) is exact.  Chains: K = (k0,) and K = (k1,)."""
    def f(Al, U_, Vt, Ar):
        return np.tensordot(Al, U_, axes=(2, 0)), np.tensordot(Vt, Ar, axes=(1, 0))
    l, r = _with_abs(f, Al, U_, Vt, Ar)
    return l, r, np.diag(np.asarray(S, dtype=np.float64))


# ---------------------------------------------------------------------------------------------- csrc/marginal.hip
def env3(side, E, At, W, Ab):
    """The three-layer environment step, UNNORMALISED, and its half-product.  At (Dt, pd, Dt2), W (bl, pd, br, pu),
    Ab (Db, pu, Db2).
    side 0: E = EL (bl, Dt, Db):   out[r,x,y] = sum EL[l,t,b] At[t,d,x] W[l,d,r,u] Ab[b,u,y],   half HL[l,d,x,b] = sum_t EL[l,t,b] At[t,d,x].
            Chains: half K = (Dt,), out K = (Dt, bl pd, Db pu).
    side 1: E = ER (br, Dt2, Db2): out[l,t,b] = sum At[t,d,x] W[l,d,r,u] Ab[b,u,y] ER[r,x,y],   half HR[u,r,x,b] = sum_y ER[r,x,y] Ab[b,u,y].
            Chains: half K = (Db2,), out K = (Db2, pu br, pd Dt2).
    Returns ((out, absout), (half, abshalf))."""
    def f0(E, At, W, Ab):
        HL = np.einsum('ltb,tdx->ldxb', E, At)
        Y = np.einsum('ldxb,ldru->rxbu', HL, W)
        return np.einsum('rxbu,buy->rxy', Y, Ab), HL

    def f1(E, At, W, Ab):
        HR = np.einsum('rxy,buy->urxb', E, Ab)
        Y = np.einsum('ldru,urxb->ldxb', W, HR)
        return np.einsum('tdx,ldxb->ltb', At, Y), HR
    return _with_abs(f0 if side == 0 else f1, E, At, W, Ab)


def env3_chain(side, Dt, pd, Dt2, bl, br, pu, Db, Db2):
    """(inner dimensions of the half-product, inner dimensions of the whole step) for gamma()."""
    if side == 0:
        return (Dt,), (Dt, bl * pd, Db * pu)
    return (Db2,), (Db2, pu * br, pd * Dt2)


def pow2_split(raw):
    """(raw / 2^e, e) with e = floor(log2 max|raw|): the power-of-two normalisation that ends env3 (exact)."""
    mx = np.abs(raw).max()
    e = int(np.floor(np.log2(mx)))
    return raw / LD(2.0) ** e, e


def cell_X(HL, HR):
    """X[l,d,u,r] = sum_{x,b} HL[l,d,x,b] HR[u,r,x,b]  (bl, pd, pu, br).  Chain: K = (Dt2 Db,)."""
    def f(HL, HR):
        return np.tensordot(HL, HR, axes=((2, 3), (2, 3)))
    return _with_abs(f, HL, HR)


def _gather(F, X, dmap, rmap):
    """T[s,l,u] = F[s,l,u] X[l,dmap[s],u,rmap[s]], 0 for the states whose dmap / rmap is out of range."""
    q = F.shape[0]
    pd, br = X.shape[1], X.shape[3]
    dmap, rmap = np.asarray(dmap, dtype=np.int64), np.asarray(rmap, dtype=np.int64)
    ok = (dmap >= 0) & (dmap < pd) & (rmap >= 0) & (rmap < br)
    T = np.zeros(F.shape, dtype=LD)
    s = np.nonzero(ok)[0]
    T[s] = F[s] * X[:, dmap[s], :, rmap[s]]                        # advanced indices first: (n, l, u)
    assert T.shape[0] == q
    return T


def cell_products(HL, HR, F, dmap, rmap):
    """(T, absT) with T[s,l,u] = F[s,l,u] X[l,dmap[s],u,rmap[s]]: every output of the two marginal steps is a sum of these."""
    X, aX = cell_X(HL, HR)
    return _gather(_ld(F), X, dmap, rmap), _gather(np.abs(_ld(F)), aX, dmap, rmap)


def marginal_chain(bl, pu, K):
    """Inner dimensions of raw p_s = sum_{l,u} F X: the X product over K = Dt2 Db, then the (l, u) sum."""
    return (K, bl * pu)


def negative_rule(raw):
    """(P, minP) of the raw table: the rule of tests/marginals_ref.py (the restatement the whole-pass tests use)."""
    return mr._negative_rule(np.asarray(raw, dtype=np.float64))


def lifted(raw):
    """The table the normalisation divides: entries below |min| lifted to |min| when min < 0 (longdouble)."""
    p = np.array(raw, dtype=LD)
    mn = p.min()
    if mn < 0:
        p[p < -mn] = -mn
    return p


def cluster_marginal(HL, HR, F, dmap, rmap, log2L=0.0, log2R=0.0):
    """dict: raw p_s and absraw (longdouble), P and minP after the negative rule (float64, uniform and -1 for an all-zero table),
    P_ld = the same table divided in longdouble (what the bounds are measured from: the float64 rule rounds a few times itself),
    log2z = log2(sum raw) + log2L + log2R, lifted_total = the sum the normalisation divides by."""
    T, aT = cell_products(HL, HR, F, dmap, rmap)
    raw, absraw = T.sum(axis=(1, 2)), aT.sum(axis=(1, 2))
    P, minP = negative_rule(raw)
    tot = raw.sum()
    with np.errstate(divide='ignore', invalid='ignore'):
        log2z = float(np.log2(tot) + LD(log2L) + LD(log2R)) if tot > 0 else float('-inf')
    lt = lifted(raw)
    P_ld = lt / lt.sum() if lt.sum() > 0 else _ld(P)
    return dict(raw=raw, absraw=absraw, P=P, P_ld=P_ld, minP=float(minP), log2z=log2z, lifted_total=lt.sum())


def marginal_bounds(ref, g):
    """(bound on |dP_s|, bound on |dlog2z|) of the module docstring from a cluster_marginal() dict and g = gamma(chain)."""
    delta = g * ref['absraw']
    sd = delta.sum()
    bP = (delta + ref['P_ld'] * sd) / ref['lifted_total']
    blz = (sd / ref['raw'].sum()) / np.log(LD(2.0)) + 4 * U * abs(ref['log2z'])
    return bP.astype(np.float64), float(blz)


def cluster_bond_marginal(HL, HR, F, dmap, rmap, log2L=0.0, log2R=0.0):
    """dict: Pl (q, bl) = sum_u T / Tot, Pu (q, pu) = sum_l T / Tot, their raw and abs-raw tables (all longdouble),
    Tot = sum T, minB = min(0, smallest entry), log2z.  An all-zero total gives uniform tables and minB = -1."""
    T, aT = cell_products(HL, HR, F, dmap, rmap)
    rl, ru = T.sum(axis=2), T.sum(axis=1)
    al, au = aT.sum(axis=2), aT.sum(axis=1)
    tot = rl.sum()
    if tot > 0:
        Pl, Pu = rl / tot, ru / tot
        minB = min(0.0, float(Pl.min()), float(Pu.min()))
        log2z = float(np.log2(tot) + LD(log2L) + LD(log2R))
    else:
        Pl, Pu = np.full(rl.shape, 1.0 / rl.size), np.full(ru.shape, 1.0 / ru.size)
        minB, log2z = -1.0, float('-inf')
    return dict(Pl=Pl, Pu=Pu, rawl=rl, rawu=ru, absl=al, absu=au, total=tot, minB=minB, log2z=log2z)


def bond_bounds(ref, gl, gu):
    """(bound on |dPl|, bound on |dPu|, bound on |dlog2z|): gl = gamma(K, pu) for the entries of Pl, gu = gamma(K, bl) for
    those of Pu; the total is the sum of the raw Pl."""
    dl, du = gl * ref['absl'], gu * ref['absu']
    sd = dl.sum()
    bl_ = (dl + np.abs(_ld(ref['Pl'])) * sd) / ref['total']
    bu_ = (du + np.abs(_ld(ref['Pu'])) * sd) / ref['total']
    blz = (sd / ref['total']) / np.log(LD(2.0)) + 4 * U * abs(ref['log2z'])
    return bl_.astype(np.float64), bu_.astype(np.float64), float(blz)


# ---------------------------------------------------------------------------------------------- inputs of the marginal cases
# (q, bl, pd, br, pu, Dt2, Db).  The CPU test asserts the preconditions of the bounds on exactly these inputs (same seeds) and
# the GPU test runs the kernels on them: the reference alone decides whether a seed is usable.
CM_SHAPES = [(40, 5, 3, 7, 6, 9, 11), (256, 16, 16, 16, 16, 8, 9), (8192, 2, 3, 5, 4, 3, 2), (16384, 2, 2, 2, 2, 2, 3)]
CM_NEGATIVE = ((40, 5, 3, 7, 6, 9, 11), 6)                          # (shape, seed) of the negative-rule case
BOND_SHAPES = [(7, 5, 2, 4, 3, 6, 9), (6, 17, 3, 5, 16, 4, 7), (5, 33, 2, 3, 7, 4, 6), (5, 3, 2, 4, 257, 6, 7), (6, 90, 3, 2, 1, 5, 4),
               (5, 2, 3, 4, 300, 7, 6)]


def marginal_seed(shape):
    return 1000 + sum((i + 1) * int(d) for i, d in enumerate(shape))


def marginal_inputs(shape, seed, kind='positive', bad_maps=False):
    """(HL (bl, pd, Dt2, Db), HR (pu, br, Dt2, Db), F (q, bl, pu), dmap, rmap int32) of one case.  kind 'positive': all operands
    in [0.1, 1.1);  'signed': HL / HR normal with a small positive mean, so that some raw sums are negative while the total
    stays positive;  'zero': F = 0.  bad_maps puts -1 and pd / br into a few entries of the maps."""
    q, bl, pd, br, pu, Dt2, Db = shape
    rng = np.random.default_rng(seed)
    if kind == 'signed':
        HL = rng.standard_normal((bl, pd, Dt2, Db)) + 0.15
        HR = rng.standard_normal((pu, br, Dt2, Db)) + 0.15
    else:
        HL = rng.uniform(0.1, 1.1, (bl, pd, Dt2, Db))
        HR = rng.uniform(0.1, 1.1, (pu, br, Dt2, Db))
    F = rng.uniform(0.1, 1.1, (q, bl, pu))
    if kind == 'zero':
        F = np.zeros_like(F)
    dmap = rng.integers(0, pd, q).astype(np.int32)
    rmap = rng.integers(0, br, q).astype(np.int32)
    if bad_maps:
        dmap[1 % q], dmap[q // 2] = -1, pd
        rmap[3 % q], rmap[q - 1] = -1, br
    return HL, HR, F, dmap, rmap


def bad_states(shape):
    """The states marginal_inputs(bad_maps=True) sends out of range."""
    q = shape[0]
    return sorted({1 % q, q // 2, 3 % q, q - 1})
