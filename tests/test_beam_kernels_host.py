"""CPU checks of tests/beam_kernels_ref.py: the references of the beam-side kernels against the oracle and against hand-worked results,
the conditions the seeded cases must meet (no comparison that could flip within the error bounds, the regime and the LDS size each
name claims), and float64 emulations of the kernels' order of operations against the error bounds the GPU test asserts."""
import math

import numpy as np
import pytest

import beam_kernels_ref as bk
from oracle import mps_ref
from oracle import solver_ref as sr

GENERIC = [n for n in bk.PN_CASES if not n.startswith('exact')]
KIB = 1024


# ------------------------------------------------------------------------------------------------------------ the table of pn.h
@pytest.mark.parametrize('name', GENERIC)
def test_pn_table_ref_agrees_with_the_oracle(name):
    """pn_table_ref against the oracle's conditional_probabilities (its _calculate_Pn, tnac4o.py:1786-1807) to 1e-13."""
    c = bk.pn_case(name)
    for b, ref in zip(c.branches, bk.pn_case_refs(name)):
        P, mP = sr.RefSolver.conditional_probabilities(c.F[:, b[2], b[3]].copy(), c.dmap, c.rmap, np.ones(1), c.T1[b[0]][None], c.RR[b[1]])
        assert np.all(np.abs(P - ref.P) <= 1e-13 * np.abs(ref.P)), (name, b)
        assert abs(mP - ref.minP) <= 1e-13 * abs(ref.minP), (name, b)


@pytest.mark.parametrize('name', list(bk.PN_CASES))
def test_pn_cases_are_unambiguous_and_in_their_regime(name):
    """No entry of any case can change sides of the lift within the error bounds, and every branch is in the regime it is listed under:
    'positive', 'partial' (0 < count < q and -1 < minP < 0), 'dominated' (everything lifted: uniform, minP = -1) or 'zero'."""
    c = bk.pn_case(name)
    q = c.shape[0]
    seen = set()
    for b, want, ref in zip(c.branches, c.regimes, bk.pn_case_refs(name)):
        assert ref.ambiguous == 0, (name, b)
        assert bk.regime_of(ref) == want, (name, b, bk.regime_of(ref))
        seen.add(want)
        if want == 'dominated':
            assert ref.count == q and abs(ref.minP + 1.0) <= ref.tol_min and np.all(np.abs(ref.P - 1.0 / q) <= ref.tol)
        if want == 'zero':
            assert ref.minP == -1.0 and np.all(ref.P == 1.0 / q) and not ref.tol.any() and ref.tol_min == 0.0
        if want == 'partial':
            assert 0 < ref.count < q and -1.0 < ref.minP < 0.0
        if want == 'positive':
            assert ref.count == 0 and ref.minP >= 0.0 and (q < 8 or np.any(ref.P == 0.0))      # zero entries: -inf in log2p_out
    if not c.exact:
        assert {'positive', 'dominated', 'zero'} <= seen and (q == 1 or 'partial' in seen)
        br = c.branches
        assert br[:, 0].max() == 2 and br[:, 1].max() == 2 and br[:, 2].max() == c.shape[4] - 1 and br[:, 3].max() == c.shape[5] - 1
        assert len(set(br[:, 0])) < len(br) and len(set(br[:, 1])) < len(br)                    # branches share prefixes and suffixes
        assert c.base[0] == 0.0 and c.base[1] == -math.inf and np.all(c.base <= 0)
        assert c.dmap.max() == c.shape[1] - 1 and c.rmap[-1] == c.shape[3] - 1


def test_pn_cases_sit_where_their_names_say():
    lds = {n: bk.calc_pn_lds(*bk.PN_CASES[n][0][:4]) for n in bk.PN_CASES}
    assert lds['lds48k_below'] == 48 * KIB and lds['lds48k_above'] == 48 * KIB + 8
    assert lds['lds64k_below'] == 64 * KIB and lds['lds64k_above'] == 64 * KIB + 8
    assert lds['lds150k_limit'] == bk.LDS_LIMIT and bk.calc_pn_lds(*bk.PN_REFUSED['refused_calc'][0][:4]) == bk.LDS_LIMIT + 8
    assert lds['workload'] <= 48 * KIB and lds['chi128'] <= 48 * KIB
    s = {n: bk.sample_pn_lds(*bk.PN_CASES[n][0][:4]) for n in bk.PN_CASES}
    assert s['sample48k_below'] == 48 * KIB and s['sample48k_above'] == 48 * KIB + 16
    assert s['sample150k_limit'] == bk.LDS_LIMIT and bk.sample_pn_lds(*bk.PN_REFUSED['refused_sample'][0][:4]) == bk.LDS_LIMIT + 16
    assert [bk.PN_CASES[n][0][0] for n in ('stride255', 'stride256', 'stride257')] == [255, 256, 257]
    nl, nu = bk.PN_CASES['nl_ne_nu'][0][4:]
    assert nl != nu


@pytest.mark.parametrize('name', ['exact12', 'exact384'])
def test_exact_cases_are_exact(name):
    """Small integers, total a power of two: four of every twelve entries equal |min| and are NOT lifted (the '<' is strict), four are;
    the table and the flag are exact in float64."""
    c = bk.pn_case(name)
    q = c.shape[0]
    ref = bk.pn_case_refs(name)[0]
    assert np.array_equal(ref.raw, np.tile(bk.EXACT_RAW, q // 12))
    assert ref.count == q // 3 and int(np.sum(ref.raw == 2.0)) == q // 3
    assert ref.no == 32.0 * (q // 12) and math.frexp(ref.no)[0] == 0.5
    assert not ref.P_lo.any() and ref.minP == -0.25 and ref.minP_lo == 0.0
    assert np.array_equal(ref.P, np.where(np.tile(bk.EXACT_RAW, q // 12) == 4, 4.0, 2.0) / ref.no)
    P, mP = bk.pn_table_emul(c.T1[0], c.RR[0], c.F, c.dmap, c.rmap, 0, 0)
    assert np.array_equal(P, ref.P) and mP == -0.25


@pytest.mark.parametrize('name', list(bk.PN_CASES))
def test_pn_emulation_within_the_bound(name):
    """The kernel's order of operations in float64 stays within 1 x tol of the 40-digit table (the GPU test asserts 2 x tol)."""
    c = bk.pn_case(name)
    worst = 0.0
    for b, ref in zip(c.branches, bk.pn_case_refs(name)):
        P, mP = bk.pn_table_emul(c.T1[b[0]], c.RR[b[1]], c.F, c.dmap, c.rmap, int(b[2]), int(b[3]))
        rP, rm = bk.pn_error_ratios(ref, P, mP)
        assert rP <= 1.0 and rm <= 1.0, (name, b, rP, rm)
        worst = max(worst, rP, rm)
    print('%s: worst error / tol of the emulation %.3f' % (name, worst))


def test_block_sum_emul_is_the_strided_tree():
    x = np.arange(1.0, 601.0)
    assert bk.block_sum_emul(x) == x.sum() and bk.block_sum_emul(x[:1]) == 1.0
    y = np.zeros(257)
    y[0], y[1], y[256] = 1.0, 2.0 ** -53, 2.0 ** -53           # thread 0 adds x[0] + x[256] first (lost), then the tree adds x[1] (lost)
    assert bk.block_sum_emul(y) == 1.0
    y[0], y[1] = 2.0 ** -53, 1.0                                # thread 0 holds x[0] + x[256] = 2^-52, which survives next to thread 1's 1.0
    assert bk.block_sum_emul(y) == 1.0 + 2.0 ** -52 and float(np.cumsum(y)[-1]) == 1.0


def test_log2p_ref():
    got = bk.log2p_ref(np.array([1.0, 0.5, 0.0, 2.0 ** -1000, 3.0]), -2.0)
    assert np.array_equal(got[:4], [-2.0, -3.0, -math.inf, -1002.0]) and abs(got[4] - (np.log2(3.0) - 2.0)) <= 2.0 ** -52
    assert np.all(bk.log2p_ref(np.array([0.25, 0.0]), -math.inf) == -math.inf)
    assert np.array_equal(bk.ulps(np.array([1.0, np.nextafter(1.0, 2.0)]), np.array([1.0, 1.0])), [0.0, 1.0])


# ------------------------------------------------------------------------------------------------------------ tn_env_rr_batched
def _env_rr_emul(A, RR, Wu):
    """env_rr_kernel's order in float64: V_d = RR . W_d^T by a sequential dot over br, one accumulator per output over d and x'."""
    Dl, p, Dr = A.shape
    bl, _, br = Wu.shape
    acc = np.zeros((Dl, bl))
    for d in range(p):
        V = np.zeros((Dr, bl))
        for c in range(br):
            V = V + RR[:, c:c + 1] * Wu[:, d, c][None, :]
        for c in range(Dr):
            acc = acc + A[:, d, c:c + 1] * V[c:c + 1, :]
    return acc


@pytest.mark.parametrize('name', list(bk.ENV_RR_CASES))
def test_env_rr_cases(name):
    """The shape takes the paths its name claims; the normalisation of no key is within the bounds of another power of two; the kernel's
    order in float64 stays within 1 x bound of the exact contraction, and so do the reference's two tensordots."""
    c = bk.env_rr_case(name)
    Dl, p, Dr, bl, br, pu = c.shape
    lds = bk.env_rr_lds(p, Dr, bl, br)
    assert Dl * bl <= 2048 and lds <= bk.LDS_LIMIT
    assert {'chi128': Dl * bl == 2048 and lds == 64 * KIB, 'partial_slot': Dl * bl == 1808 and (Dl * bl) % 256 != 0,
            'slot5': Dl * bl == 1040, 'lds96k': lds == 96 * KIB,
            'lds150k_limit': bk.env_rr_lds(p + 1, Dr, bl, br) > bk.LDS_LIMIT}[name]
    refs = bk.env_rr_case_refs(name)
    assert refs[0].expo is None and not refs[0].hi.any()                    # the zero parent
    worst = 0.0
    for k in (1, 2):
        ref = refs[k]
        assert ref.ambiguous == 0 and ref.expo is not None
        RR, Wu = c.RRp[c.parent[k]], c.W[:, :, :, c.uidx[k]]
        for got in (_env_rr_emul(c.A, RR, Wu), np.tensordot(np.tensordot(c.A, RR, axes=(2, 0)), Wu, axes=([1, 2], [1, 2]))):
            r = bk.env_rr_error_ratio(ref, np.ldexp(got, -ref.expo))
            assert r <= 1.0, (name, k, r)
            worst = max(worst, r)
        assert mps_ref.pow2_floor_max(ref.hi) == 2.0 ** ref.expo
    print('%s: worst error / bound of the emulations %.4f' % (name, worst))
    for shape, _ in bk.ENV_RR_REFUSED.values():
        assert shape[0] * shape[3] == 2049 or bk.env_rr_lds(shape[1], shape[2], shape[3], shape[4]) > bk.LDS_LIMIT


def test_env_rr_exact_against_mpmath():
    """The integer evaluation against a plain mpmath sum at 40 digits, on the smallest case."""
    import mpmath
    c = bk.env_rr_case('slot5')
    Dl, p, Dr, bl, br, pu = c.shape
    ref = bk.env_rr_case_refs('slot5')[2]
    RR, Wu = c.RRp[c.parent[2]], c.W[:, :, :, c.uidx[2]]
    with mpmath.workdps(bk.DPS):
        f = lambda x: mpmath.mpf(float(x))      # noqa: E731
        for x, l in ((0, 0), (17, 5), (Dl - 1, bl - 1)):
            s = mpmath.fsum(f(c.A[x, d, y]) * f(RR[y, r]) * f(Wu[l, d, r]) for d in range(p) for y in range(Dr) for r in range(br))
            assert abs(s - (f(ref.hi[x, l]) + f(ref.lo[x, l]))) <= abs(s) * mpmath.mpf(10) ** -30


# ------------------------------------------------------------------------------------------------------------ bit-for-bit references
def test_merge_groups_ref_by_hand():
    c = bk.merge_case('window_zero')
    rep, dn, ln = bk.merge_groups_ref(c.E, c.lp, c.deg, c.pos, c.starts, c.min_dEng)
    s = c.starts
    first = (0, 1, 0, 1, 0, 0, 0, 0)                             # the FIRST of the minima
    assert [int(x) for x in rep] == [int(c.pos[s[g] + o]) for g, o in enumerate(first)]
    assert [int(x) for x in dn] == [3, 2 + 3 + 5, 7 + 17, 1, 6, 4, 4, 2 ** 62 + 2 ** 60 + 5]
    assert np.signbit(ln[0]) and ln[0] == 0.0 and np.signbit(ln[3]) and ln[3] == 0.0           # alone: its own -0.0, not 0.0 + -0.0
    assert ln[1] == (-2.0 + -5.0 + -11.0) / 3 and ln[2] == (-3.0 + -6.5) / 2
    assert ln[4] == -math.inf and ln[5] == -3.5 and ln[6] == -math.inf and ln[7] == -2.5
    c = bk.merge_case('window_edge')
    rep, dn, ln = bk.merge_groups_ref(c.E, c.lp, c.deg, c.pos, c.starts, c.min_dEng)
    assert [int(x) for x in rep] == [int(c.pos[c.starts[g] + o]) for g, o in enumerate(first)]
    assert int(dn[2]) == 7 + 11 + 17 and ln[2] == (-3.0 + -4.0 + -6.5) / 3                      # E = Emin + min_dEng is in, one ulp more is out
    c = bk.merge_case('empty_mixed')
    rep, dn, ln = bk.merge_groups_ref(c.E, c.lp, c.deg, c.pos, c.starts, c.min_dEng)
    empty = np.diff(c.starts) == 0
    assert list(empty) == [False, True, False, True, True, False, True]
    assert np.all(rep[empty] == -1) and np.all(dn[empty] == 0) and np.all(ln[empty] == -math.inf) and np.all(rep[~empty] >= 0)


@pytest.mark.parametrize('name', bk.MERGE_CASES)
def test_merge_cases(name):
    c = bk.merge_case(name)
    sizes = np.diff(c.starts)
    assert c.ng == sizes.size == int(name[2:]) if name[2:].isdigit() else c.ng == sizes.size
    assert c.E.size == c.lp.size == c.deg.size == c.pos.size == c.starts[-1]
    assert (name in bk.MERGE_EMPTY) == bool(np.any(sizes == 0)) and (name not in bk.MERGE_EMPTY or sizes[-1] == 0)
    if name in ('ng1', 'ng255', 'ng256', 'ng257'):
        assert sizes.max() == 1000 and (c.ng == 1 or sizes.min() == 1)
    if name not in ('generic', 'empty_only'):                    # ties, and members exactly at the edge of the window, do occur
        d = np.concatenate([c.E[a:b] - c.E[a:b].min() for a, b in zip(c.starts[:-1], c.starts[1:]) if b > a])
        assert np.sum(d == 0) > np.sum(sizes > 0) and (c.min_dEng == 0.0 or np.any(d == c.min_dEng))


def test_env_rl_and_nfactor_refs():
    for Dr in bk.ENV_RL_DR:
        T1, par, didx = bk.env_rl_case(Dr, 5, 0)
        assert (par[0], didx[0]) == (1, 1) and (par[1], didx[1]) == (2, 0) and (par[2], didx[2]) == (3, 2)
        assert 0 < np.abs(T1[2, 0]).max() < 2.0 ** -1022
        out = bk.env_rl_ref(T1, par, didx)
        assert not out[0].any() and np.array_equal(out[1], T1[2, 0] * 2.0 ** 1023)
        assert 1.0 <= np.abs(out[2]).max() < 2.0
    assert {tuple(bk.env_rl_case(7, 1, f)[1]) for f in range(3)} == {(1,), (2,), (3,)}
    for n in bk.NFACTOR_LEN:
        X = np.stack([bk.nfactor_block(k, n, 0) for k in bk.NFACTOR_KINDS])
        out = bk.nfactor_batched_ref(X)
        assert not out[0].any() and np.array_equal(out[1], X[1] * 2.0 ** 1023) and 0 < np.abs(X[1]).max() < 2.0 ** -1022
        assert 1.0 <= np.abs(out[2]).max() < 2.0 and np.array_equal(out[2] * mps_ref.pow2_floor_max(X[2]), X[2])
