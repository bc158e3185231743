"""The composed site and environment steps (tnac4o_amd.ops over tn_rar, tn_env_mix, tn_apply_truncation, tn_env3,
tn_cluster_marginal, tn_cluster_bond_marginal) against the longdouble references of tests/steps_ref.py.

The other direct tests of these entry points compare them with their own wrappers (workspace contracts) and the whole-pass tests
run them at symmetric shapes (bulk bonds all chi, bl = br, pd = pu), where a swapped index pair or a wrong stride between two
equal dimensions passes.  Here all dimensions of a case are pairwise distinct wherever the signature allows, operands are signed
(positive only where a relative bound on a normalised table needs it), and bond_gather_kernel / cluster_marginal_kernel run at
the shapes that take their other paths: pu that does not divide 256, pu > 256 (two column tiles), bl > 256 / pu, q 8 > 48 KiB.

Bounds: steps_ref's (derived, no safety factor): |got - ref| <= gamma(chain) absref for the products, and for the normalised
tables |dP_s| <= (delta_s + P_s sum(delta)) / sum_lifted, |dlog2z| <= (sum(delta) / raw) / ln 2 + 4 u |log2z| with
delta_s = gamma absraw_s.  The preconditions (positive raw totals; for the negative rule a negative minimum, no entry within
1e-6 |min| of the threshold, lifted total above |min|) are asserted on the same inputs by tests/test_steps_ref_host.py.

Every bounded case prints its largest error / bound (pytest -s); a ratio near 1 would mean the bound does no work, above 1 fails.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
import steps_ref as sr  # noqa: E402

F64 = torch.float64
LD = np.longdouble


@pytest.fixture(scope='module')
def ops():
    from tnac4o_amd import ops as o
    return o


def dev(x, dtype=F64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).cuda()


def host(t):
    return t.detach().cpu().numpy()


def normal(rng, *shape):
    return rng.standard_normal(shape)


RATIOS = {}


def within(name, got, ref, bound):
    """|got - ref| <= bound elementwise (bound > 0 everywhere); prints the largest error / bound (recorded in the module docstring)."""
    got = np.asarray(got)
    assert got.shape == np.shape(ref), (name, got.shape, np.shape(ref))
    assert np.all(np.isfinite(got)), name
    err = np.abs(np.asarray(got, dtype=LD) - np.asarray(ref, dtype=LD))
    bound = np.asarray(bound, dtype=LD)
    assert np.all(bound > 0), name
    ratio = float((err / bound).max())
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print('error/bound %-28s %.3f (largest so far %.3f)' % (name, ratio, RATIOS[name]))
    assert ratio <= 1.0, (name, ratio)


# ------------------------------------------------------------------------------------------------------------------ csrc/site.hip
@pytest.mark.parametrize('c,a,s,a2,c2', [(33, 31, 4, 65, 63), (5, 7, 3, 2, 11), (1, 70, 2, 66, 1)])
def test_rar(ops, c, a, s, a2, c2):
    rng = np.random.default_rng(c + 2 * a + 3 * s)
    RL, A, RR = normal(rng, c, a), normal(rng, a, s, a2), normal(rng, a2, c2)
    got = host(ops.rar(dev(RL), dev(A), dev(RR)))
    ref, absref = sr.rar(RL, A, RR)
    within('rar', got, ref, sr.gamma(a, a2) * absref)


@pytest.mark.parametrize('side', (0, 1))
@pytest.mark.parametrize('a,s,a2,c,c2', [(33, 4, 31, 65, 63), (7, 3, 5, 2, 11), (70, 2, 66, 1, 1)])
def test_env_mix(ops, side, a, s, a2, c, c2):
    rng = np.random.default_rng(a + 2 * s + 3 * c + side)
    A, Ac = normal(rng, a, s, a2), normal(rng, c, s, c2)
    R = normal(rng, c, a) if side == 0 else normal(rng, a2, c2)
    got = host(ops.env_mix(side, dev(R), dev(A), dev(Ac)))
    ref, absref = sr.env_mix(side, R, A, Ac)
    within('env_mix', got, ref, (sr.gamma(a, c * s) if side == 0 else sr.gamma(a2, s * c2)) * absref)


@pytest.mark.parametrize('Dl,p,k0,keep,k1,p2,Dr,u_transposed', [(16, 4, 33, 31, 65, 2, 63, False), (3, 2, 7, 5, 11, 4, 1, False),
                                                              (16, 4, 33, 31, 65, 2, 63, True)])
def test_apply_truncation(ops, Dl, p, k0, keep, k1, p2, Dr, u_transposed):
    """U and Vt are the leading columns / rows of the factors of a larger decomposition, as the sweeps pass them: strided views."""
    rng = np.random.default_rng(Dl + k0 + keep)
    Al, Ar, S = normal(rng, Dl, p, k0), normal(rng, k1, p2, Dr), np.sort(rng.random(keep))[::-1].copy()
    Ufull, Vfull = normal(rng, k0, keep + 3), normal(rng, keep + 2, k1)
    if u_transposed:
        Ud = dev(Ufull.T).t()[:, :keep]
        assert Ud.stride() == (1, k0)
    else:
        Ud = dev(Ufull)[:, :keep]
        assert Ud.stride() == (keep + 3, 1)
    Vd = dev(Vfull)[:keep]
    Aln, Arn, Cd = ops.apply_truncation(dev(Al), Ud, dev(S), Vd, dev(Ar))
    (l, al), (r, ar), Cref = sr.apply_truncation(Al, Ufull[:, :keep], S, Vfull[:keep], Ar)
    within('apply_truncation', host(Aln), l, sr.gamma(k0) * al)
    within('apply_truncation', host(Arn), r, sr.gamma(k1) * ar)
    assert np.array_equal(host(Cd), Cref)


# ------------------------------------------------------------------------------------------------------------------ tn_env3
ENV3_SHAPES = [(33, 4, 31, 3, 5, 2, 17, 65), (7, 5, 3, 4, 2, 6, 9, 11), (64, 2, 66, 2, 3, 4, 62, 70)]      # Dt, pd, Dt2, bl, br, pu, Db, Db2


@pytest.fixture(scope='module')
def env3_cases():
    """Inputs and longdouble references of every (shape, side), computed once for the keep_half / log2nf_in variants."""
    cases = {}
    for shape in ENV3_SHAPES:
        Dt, pd, Dt2, bl, br, pu, Db, Db2 = shape
        for side in (0, 1):
            rng = np.random.default_rng(sum(shape) + side)
            At, W, Ab = normal(rng, Dt, pd, Dt2), normal(rng, bl, pd, br, pu), normal(rng, Db, pu, Db2)
            E = normal(rng, bl, Dt, Db) if side == 0 else normal(rng, br, Dt2, Db2)
            cases[shape, side] = (E, At, W, Ab) + sr.env3(side, E, At, W, Ab)
    return cases


@pytest.mark.parametrize('lg_in', (None, 12.0))
@pytest.mark.parametrize('keep_half', (False, True))
@pytest.mark.parametrize('side', (0, 1))
@pytest.mark.parametrize('shape', ENV3_SHAPES)
def test_env3(ops, env3_cases, shape, side, keep_half, lg_in):
    E, At, W, Ab, (raw, absraw), (half, abshalf) = env3_cases[shape, side]
    kh, ko = sr.env3_chain(side, *shape)
    res = ops.env3(side, dev(E), dev(At), dev(W), dev(Ab), log2nf_in=None if lg_in is None else dev(np.array([lg_in])), keep_half=keep_half)
    out, lg = host(res[0]), float(host(res[1])[0])
    assert out.shape == raw.shape
    assert 1.0 <= np.abs(out).max() < 2.0
    e = lg - (lg_in or 0.0)
    assert e == np.floor(e)
    within('env3', np.asarray(out, dtype=LD) * LD(2.0) ** int(e), raw, sr.gamma(*ko) * absraw)
    if keep_half:
        within('env3 half', host(res[2]), half, sr.gamma(*kh) * abshalf)


# ------------------------------------------------------------------------------------------------------------------ tn_cluster_marginal
def _marginal(ops, ins, lgs=(None, None)):
    HL, HR, F, dmap, rmap = ins
    P, mP, lz = ops.cluster_marginal(dev(HL), dev(HR), dev(F), dev(dmap, torch.int32), dev(rmap, torch.int32),
                                     *[None if x is None else dev(np.array([x])) for x in lgs])
    return host(P), float(host(mP)[0]), float(host(lz)[0])


def _check_marginal(shape, ins, got, lgs=(0.0, 0.0)):
    q, bl, pd, br, pu, Dt2, Db = shape
    P, mP, lz = got
    ref = sr.cluster_marginal(*ins, *lgs)
    bP, blz = sr.marginal_bounds(ref, sr.gamma(*sr.marginal_chain(bl, pu, Dt2 * Db)))
    zero = ref['absraw'] == 0                                            # states the maps send out of range: raw 0 exactly
    if not (ref['raw'].min() < 0):
        assert np.all(P[zero] == 0.0)
    within('cluster_marginal P', P[~zero], ref['P_ld'][~zero], bP[~zero])
    within('cluster_marginal log2z', [lz], [ref['log2z']], [blz])
    return ref, bP


@pytest.mark.parametrize('bad_maps', (False, True))
@pytest.mark.parametrize('shape', sr.CM_SHAPES)
def test_cluster_marginal_positive(ops, shape, bad_maps):
    """q 8 bytes of LDS: 320 B, 2 KiB, 64 KiB (above the 48 KiB a kernel gets without asking) and the limit, 128 KiB."""
    ins = sr.marginal_inputs(shape, sr.marginal_seed(shape), 'positive', bad_maps)
    got = _marginal(ops, ins)
    ref, _ = _check_marginal(shape, ins, got)
    assert got[1] >= 0.0                                                 # no negative entry: the flag is min P
    bad = sr.bad_states(shape) if bad_maps else []
    assert np.all(got[0][bad] == 0.0) and got[1] == (0.0 if bad_maps else got[0].min())


def test_cluster_marginal_log2_totals(ops):
    shape = sr.CM_SHAPES[0]
    ins = sr.marginal_inputs(shape, sr.marginal_seed(shape), 'positive')
    plain = _marginal(ops, ins)
    for lgs in ((37.0, None), (None, -5.0), (37.0, -5.0)):
        got = _marginal(ops, ins, lgs)
        _check_marginal(shape, ins, got, tuple(x or 0.0 for x in lgs))
        assert np.array_equal(got[0], plain[0]) and got[1] == plain[1]
        assert got[2] == plain[2] + (lgs[0] or 0.0) + (lgs[1] or 0.0)      # (added in this order by the kernel; 37 and -5 are exact)


def test_cluster_marginal_negative_rule(ops):
    shape, seed = sr.CM_NEGATIVE
    ins = sr.marginal_inputs(shape, seed, 'signed')
    P, mP, lz = got = _marginal(ops, ins)
    ref, bP = _check_marginal(shape, ins, got)
    raw = ref['raw']
    a = -raw.min()
    low = np.asarray(raw < a)
    assert low.sum() >= 2 and (~low).sum() >= 2
    assert np.all(P[low] == P[low][0]) and np.all(P[~low] > P[low][0])    # the lifted entries are one value, the smallest
    # minP = -(number lifted) x the lifted value |min| / lifted total, i.e. -(number lifted) x P of the minimal state
    s = int(np.argmin(raw))
    within('cluster_marginal P', [mP], [-int(low.sum()) * ref['P_ld'][s]], [int(low.sum()) * bP[s]])


def test_cluster_marginal_all_zero(ops):
    shape = sr.CM_SHAPES[0]
    P, mP, lz = _marginal(ops, sr.marginal_inputs(shape, 3, 'zero'))
    assert np.array_equal(P, np.full(shape[0], 1.0 / shape[0])) and mP == -1.0


def test_cluster_marginal_rejects_too_many_states(ops):
    from tnac4o_amd._lib import TnError
    q, bl, pd, br, pu, Dt2, Db = 16385, 2, 2, 2, 2, 2, 3
    z = torch.zeros
    with pytest.raises(TnError, match='more than 16384 cell states'):
        ops.cluster_marginal(z((bl, pd, Dt2, Db), dtype=F64, device='cuda'), z((pu, br, Dt2, Db), dtype=F64, device='cuda'),
                             z((q, bl, pu), dtype=F64, device='cuda'), z(q, dtype=torch.int32, device='cuda'),
                             z(q, dtype=torch.int32, device='cuda'))


# ------------------------------------------------------------------------------------------------------------------ tn_cluster_bond_marginal
def _bond(ops, ins, lgs=(None, None)):
    HL, HR, F, dmap, rmap = ins
    Pl, Pu, mB, lz = ops.cluster_bond_marginal(dev(HL), dev(HR), dev(F), dev(dmap, torch.int32), dev(rmap, torch.int32),
                                               *[None if x is None else dev(np.array([x])) for x in lgs])
    return host(Pl), host(Pu), float(host(mB)[0]), float(host(lz)[0])


@pytest.mark.parametrize('bad_maps', (False, True))
@pytest.mark.parametrize('shape', sr.BOND_SHAPES, ids=lambda s: 'bl%d-pu%d' % (s[1], s[4]))
def test_cluster_bond_marginal_positive(ops, shape, bad_maps):
    """(bl, pu): TU = pu, TL = 256 / pu rows per tile -- 3 | 85, 16 | 16 (bl = 17: two row tiles), 7 | 36 (256 = 7 * 36 + 4 idle
    lanes), 257 and 300 (two column tiles of 256, Pl added up across them), 1 | 256 (bl = 90 in one tile)."""
    q, bl, pd, br, pu, Dt2, Db = shape
    ins = sr.marginal_inputs(shape, sr.marginal_seed(shape), 'positive', bad_maps)
    Pl, Pu, mB, lz = _bond(ops, ins, (3.0, None))
    ref = sr.cluster_bond_marginal(*ins, 3.0, 0.0)
    K = Dt2 * Db
    bl_, bu_, blz = sr.bond_bounds(ref, sr.gamma(K, pu), sr.gamma(K, bl))
    bad = sr.bad_states(shape) if bad_maps else []
    good = np.setdiff1d(np.arange(q), bad)
    assert np.all(Pl[bad] == 0.0) and np.all(Pu[bad] == 0.0)
    within('cluster_bond_marginal P', Pl[good], ref['Pl'][good], bl_[good])
    within('cluster_bond_marginal P', Pu[good], ref['Pu'][good], bu_[good])
    within('cluster_bond_marginal log2z', [lz], [ref['log2z']], [blz])
    assert mB == 0.0
    Pl_, Pu_ = np.asarray(Pl, dtype=LD), np.asarray(Pu, dtype=LD)
    assert abs(float(Pl_.sum()) - 1.0) <= float(bl_.sum())
    assert np.all(np.abs(Pl_.sum(axis=1) - Pu_.sum(axis=1)) <= bl_.sum(axis=1) + bu_.sum(axis=1))


def test_cluster_bond_marginal_all_zero(ops):
    shape = sr.BOND_SHAPES[0]
    q, bl, pu = shape[0], shape[1], shape[4]
    Pl, Pu, mB, lz = _bond(ops, sr.marginal_inputs(shape, 3, 'zero'))
    assert np.array_equal(Pl, np.full((q, bl), 1.0 / (q * bl))) and np.array_equal(Pu, np.full((q, pu), 1.0 / (q * pu))) and mB == -1.0
