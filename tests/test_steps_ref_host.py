"""CPU checks of tests/steps_ref.py, the longdouble references of the composed site and environment steps.

1. Every reference against explicit Python loops over the defining formula, at the smallest shapes whose dimensions are all
   distinct (a permutation of 1 .. n for a step with n dimensions: a swapped index pair or a transposed operand cannot pass).
2. The negative-rule reference against tests/marginals_ref.py.
3. The preconditions the bounds of tests/test_gpu_steps_ref.py rest on, asserted on the very inputs (same generator, same
   seeds) the GPU cases use, so that they are verified without a GPU and decided by the reference alone:
     positive-input cases: raw total > 0 (and every raw entry > 0, so that relative bounds mean something);
     negative-rule case:   min_s p_s < 0; no p_s within 1e-6 |min| of the threshold |min| (a rounding error of the kernel cannot
                           move an entry across the rule); the lifted total exceeds |min|.
"""
import itertools

import numpy as np
import pytest

import marginals_ref as mr
import steps_ref as sr

LD = np.longdouble


def _rand(rng, *shape):
    return rng.standard_normal(shape)


def _close(got, want, absref):
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.abs(got - want) <= 1e-15 * np.asarray(absref, dtype=LD) + 1e-300)


def _loops(shape, term):
    """out[idx] = sum over the inner index ranges of term(*idx, *inner); shape = (outer dims, inner dims)."""
    outer, inner = shape
    out = np.zeros(outer, dtype=LD)
    for o in itertools.product(*[range(n) for n in outer]):
        acc = LD(0)
        for i in itertools.product(*[range(n) for n in inner]):
            acc += term(*o, *i)
        out[o] = acc
    return out


def test_rar_against_loops():
    c, a, s, a2, c2 = 3, 5, 2, 4, 1
    rng = np.random.default_rng(1)
    RL, A, RR = _rand(rng, c, a), _rand(rng, a, s, a2), _rand(rng, a2, c2)
    want = _loops(((c, s, c2), (a, a2)), lambda i, j, k, x, y: LD(RL[i, x]) * A[x, j, y] * RR[y, k])
    ref, absref = sr.rar(RL, A, RR)
    _close(ref, want, absref)
    _close(absref, sr.rar(np.abs(RL), np.abs(A), np.abs(RR))[0], absref)
    assert np.all(absref >= np.abs(ref))


@pytest.mark.parametrize('side', (0, 1))
def test_env_mix_against_loops(side):
    a, s, a2, c, c2 = 3, 2, 5, 4, 1
    rng = np.random.default_rng(2 + side)
    A, Ac = _rand(rng, a, s, a2), _rand(rng, c, s, c2)
    if side == 0:
        R = _rand(rng, c, a)
        want = _loops(((c2, a2), (c, s, a)), lambda i, j, x, y, z: LD(Ac[x, y, i]) * R[x, z] * A[z, y, j])
    else:
        R = _rand(rng, a2, c2)
        want = _loops(((a, c), (s, a2, c2)), lambda i, j, y, x, z: LD(A[i, y, x]) * R[x, z] * Ac[j, y, z])
    ref, absref = sr.env_mix(side, R, A, Ac)
    _close(ref, want, absref)
    assert np.all(absref >= np.abs(ref))


def test_apply_truncation_against_loops():
    Dl, p, k0, keep, k1, p2, Dr = 2, 3, 5, 4, 7, 1, 6
    rng = np.random.default_rng(4)
    Al, Uu, Vt, Ar, S = _rand(rng, Dl, p, k0), _rand(rng, k0, keep), _rand(rng, keep, k1), _rand(rng, k1, p2, Dr), rng.random(keep)
    (l, al), (r, ar), Cd = sr.apply_truncation(Al, Uu, S, Vt, Ar)
    _close(l, _loops(((Dl, p, keep), (k0,)), lambda i, j, k, x: LD(Al[i, j, x]) * Uu[x, k]), al)
    _close(r, _loops(((keep, p2, Dr), (k1,)), lambda i, j, k, x: LD(Vt[i, x]) * Ar[x, j, k]), ar)
    assert Cd.shape == (keep, keep) and np.array_equal(Cd, np.diag(S))


@pytest.mark.parametrize('side', (0, 1))
def test_env3_against_loops(side):
    Dt, pd, Dt2, bl, br, pu, Db, Db2 = 3, 2, 5, 4, 1, 7, 8, 6
    rng = np.random.default_rng(5 + side)
    At, W, Ab = _rand(rng, Dt, pd, Dt2), _rand(rng, bl, pd, br, pu), _rand(rng, Db, pu, Db2)
    if side == 0:
        E = _rand(rng, bl, Dt, Db)
        want = _loops(((br, Dt2, Db2), (bl, Dt, Db, pd, pu)),
                      lambda r, x, y, l, t, b, d, u: LD(E[l, t, b]) * At[t, d, x] * W[l, d, r, u] * Ab[b, u, y])
        whalf = _loops(((bl, pd, Dt2, Db), (Dt,)), lambda l, d, x, b, t: LD(E[l, t, b]) * At[t, d, x])
    else:
        E = _rand(rng, br, Dt2, Db2)
        want = _loops(((bl, Dt, Db), (pd, Dt2, br, pu, Db2)),
                      lambda l, t, b, d, x, r, u, y: LD(At[t, d, x]) * W[l, d, r, u] * Ab[b, u, y] * E[r, x, y])
        whalf = _loops(((pu, br, Dt2, Db), (Db2,)), lambda u, r, x, b, y: LD(E[r, x, y]) * Ab[b, u, y])
    (out, aout), (half, ahalf) = sr.env3(side, E, At, W, Ab)
    _close(out, want, aout)
    _close(half, whalf, ahalf)
    assert np.all(aout >= np.abs(out)) and np.all(ahalf >= np.abs(half))
    n, e = sr.pow2_split(out)
    assert 1 <= np.abs(n).max() < 2 and np.array_equal(n * LD(2.0) ** e, out)


def _marginal_loops(HL, HR, F, dmap, rmap):
    q, bl, pu = F.shape
    pd, br = HL.shape[1], HR.shape[1]
    T = np.zeros((q, bl, pu), dtype=LD)
    for s in range(q):
        d, r = int(dmap[s]), int(rmap[s])
        if not (0 <= d < pd and 0 <= r < br):
            continue
        for l in range(bl):
            for u in range(pu):
                x = LD(0)
                for t in range(HL.shape[2]):
                    for b in range(HL.shape[3]):
                        x += LD(HL[l, d, t, b]) * HR[u, r, t, b]
                T[s, l, u] = F[s, l, u] * x
    return T


@pytest.mark.parametrize('bad_maps', (False, True))
def test_cluster_marginals_against_loops(bad_maps):
    shape = (8, 3, 2, 5, 4, 6, 7)                                         # q, bl, pd, br, pu, Dt2, Db: all distinct
    HL, HR, F, dmap, rmap = sr.marginal_inputs(shape, 7, 'signed', bad_maps)
    T = _marginal_loops(HL, HR, F, dmap, rmap)
    X, aX = sr.cell_X(HL, HR)
    assert X.shape == (3, 2, 4, 5)
    _close(X[2, 1, 3, 4], sum(LD(HL[2, 1, t, b]) * HR[3, 4, t, b] for t in range(6) for b in range(7)), aX[2, 1, 3, 4])
    ref = sr.cluster_marginal(HL, HR, F, dmap, rmap, 3.0, -5.0)
    _close(ref['raw'], T.sum(axis=(1, 2)), ref['absraw'])
    if bad_maps:
        assert sr.bad_states(shape) == [1, 3, 4, 7]
        assert np.all(ref['raw'][sr.bad_states(shape)] == 0) and np.all(ref['absraw'][sr.bad_states(shape)] == 0)
    good = np.setdiff1d(np.arange(8), sr.bad_states(shape) if bad_maps else [])
    assert np.all(ref['absraw'][good] > 0)
    assert abs(ref['log2z'] - (float(np.log2(T.sum())) - 2.0)) <= 1e-13
    bond = sr.cluster_bond_marginal(HL, HR, F, dmap, rmap, 3.0, -5.0)
    _close(bond['rawl'], T.sum(axis=2), bond['absl'])
    _close(bond['rawu'], T.sum(axis=1), bond['absu'])
    tot = T.sum()
    assert np.abs(bond['Pl'] - T.sum(axis=2) / tot).max() <= 1e-15
    assert np.abs(bond['Pu'] - T.sum(axis=1) / tot).max() <= 1e-15
    assert bond['minB'] == min(0.0, float(bond['Pl'].min()), float(bond['Pu'].min())) and bond['minB'] < 0      # (signed inputs)
    assert abs(bond['log2z'] - ref['log2z']) <= 1e-13


def test_all_zero_tables_are_uniform():
    shape = (8, 3, 2, 5, 4, 6, 7)
    ins = sr.marginal_inputs(shape, 7, 'zero')
    ref = sr.cluster_marginal(*ins)
    assert np.array_equal(ref['P'], np.full(8, 1.0 / 8)) and ref['minP'] == -1.0
    bond = sr.cluster_bond_marginal(*ins)
    assert np.array_equal(bond['Pl'], np.full((8, 3), 1.0 / 24)) and np.array_equal(bond['Pu'], np.full((8, 4), 1.0 / 32))
    assert bond['minB'] == -1.0


def test_negative_rule_agrees_with_marginals_ref():
    rng = np.random.default_rng(9)
    for trial in range(20):
        raw = rng.standard_normal(12) + 0.8
        if trial == 0:
            raw = np.abs(raw)
        P, mn = sr.negative_rule(raw.astype(LD))
        P2, mn2 = mr._negative_rule(raw)
        assert np.array_equal(P, P2) and mn == mn2
        lifted = sr.lifted(raw)
        # the rule stated on its own: entries below |min| become |min|, minP = min * (number lifted) / lifted total
        m = raw.min()
        if m < 0:
            want = np.where(raw < -m, -m, raw)
            assert np.array_equal(lifted.astype(float), want)
            assert np.abs(P - want / want.sum()).max() <= 1e-15
            assert abs(mn - m * (raw < -m).sum() / want.sum()) <= 1e-15 * abs(mn)
        else:
            assert np.array_equal(lifted.astype(float), raw) and mn == m / raw.sum()
    P, mn = sr.negative_rule(np.zeros(5))
    assert np.array_equal(P, np.full(5, 0.2)) and mn == -1.0


def test_gamma():
    assert sr.gamma(3, 4) == 9 * sr.U / (1 - 9 * sr.U)
    assert sr.env3_chain(0, 1, 2, 3, 4, 5, 6, 7, 8) == ((1,), (1, 8, 42)) and sr.env3_chain(1, 1, 2, 3, 4, 5, 6, 7, 8) == ((8,), (8, 30, 6))


# ---------------------------------------------------------------------------------------------- preconditions of the GPU cases
@pytest.mark.parametrize('shape', sr.CM_SHAPES + sr.BOND_SHAPES)
@pytest.mark.parametrize('bad_maps', (False, True))
def test_positive_cases_have_positive_raw_total(shape, bad_maps):
    HL, HR, F, dmap, rmap = sr.marginal_inputs(shape, sr.marginal_seed(shape), 'positive', bad_maps)
    ref = sr.cluster_marginal(HL, HR, F, dmap, rmap)
    assert ref['raw'].sum() > 0
    bad = sr.bad_states(shape) if bad_maps else []
    good = np.setdiff1d(np.arange(shape[0]), bad)
    assert np.all(ref['raw'][good] > 0) and np.all(ref['raw'][bad] == 0)
    assert np.array_equal(ref['raw'], ref['absraw'])                     # positive operands: the bounds are relative ones
    assert ref['minP'] >= 0 and abs(ref['P'].sum() - 1) <= 1e-12
    assert np.all(np.abs(ref['P'] - ref['P_ld']) <= 8 * sr.U * ref['P_ld'])
    assert len(set(shape)) == len(shape) or shape in sr.CM_SHAPES[1:]    # (the shapes the issue fixes repeat dimensions)


def test_negative_rule_case_preconditions():
    shape, seed = sr.CM_NEGATIVE
    ref = sr.cluster_marginal(*sr.marginal_inputs(shape, seed, 'signed'))
    raw = ref['raw']
    mn = raw.min()
    assert mn < 0
    a = -mn
    assert np.all(np.abs(raw - a) > 1e-6 * a)
    assert ref['lifted_total'] > a
    assert raw.sum() > 0                                                 # log2z is defined
    assert (raw < a).sum() >= 2 and (raw > a).sum() >= 2                 # both lifted and untouched entries exist
    assert ref['minP'] < 0
    assert np.all(np.abs(ref['P'] - ref['P_ld']) <= 8 * sr.U * ref['P_ld'])       # the float64 rule and the longdouble division agree
    assert abs(ref['minP'] + (raw < a).sum() * ref['P_ld'][np.argmin(raw)]) <= 8 * sr.U * abs(ref['minP'])
