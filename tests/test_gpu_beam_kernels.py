"""The beam-side kernels on the GPU, each against the references and seeded cases of tests/beam_kernels_ref.py (checked on the CPU by
tests/test_beam_kernels_host.py): tn_calc_pn against a 40-digit table within twice its running error bound, log2p_out in ulps of the
correctly rounded value, tn_sample_pn / tn_score_pn bit for bit against tn_calc_pn at the shapes and LDS sizes the other tests leave
out, tn_env_rr_batched against the exact contraction, tn_env_rl_batched / tn_merge_groups / tn_nfactor_batched bit for bit.  Refusals
go through the C-ABI with the outputs framed by guard bytes (tests/guarded.py) and must write nothing."""
import ctypes as ct
import functools
import math

import numpy as np
import pytest

import beam_kernels_ref as bk
import sampling_ref as sref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
from guarded import Guarded, same_bits  # noqa: E402

F64 = torch.float64
SENT = 0x5A                                  # sentinel byte of outputs that must stay untouched
LOG2P_MAX_ULPS = 1.0                         # the largest distance of log2p_out from log2p_ref measured on an MI355X (see test_calc_pn_log2p)
ULP_SAMPLE = 1024                            # entries per branch whose log2 is recomputed in mpmath
SCORE_CASES = ('workload', 'chi128', 'lds48k_below', 'lds48k_above', 'lds64k_below', 'lds64k_above', 'lds150k_limit')
SAMPLE_CASES = ('workload', 'chi128', 'sample48k_below', 'sample48k_above', 'sample150k_limit')
GROUP_SIZES = (1, 300, 2, 257, 64, 5, 3, 40)


@pytest.fixture(scope='module')
def L():
    from tnac4o_amd import _lib
    return _lib.lib()


def _st():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _msg(L):
    buf = ct.create_string_buffer(256)
    L.tn_last_error(buf, 256)
    return buf.value.decode()


def dv(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    return (t.to(dtype) if dtype is not None else t).cuda()


def host(t):
    return t.cpu().numpy()


def _pn_args(c, T1=None):
    return [dv(c.T1 if T1 is None else T1), dv(c.RR), dv(c.F), dv(c.dmap), dv(c.rmap)] + [dv(c.branches[:, j].copy()) for j in range(4)]


@functools.lru_cache(maxsize=None)
def _calc(name, zero_base=False):
    """(P, minP, log2p_out) of tn_calc_pn on the case, on the host; computed once and shared."""
    from tnac4o_amd import ops
    c = bk.pn_case(name)
    base = np.zeros(len(c.branches)) if zero_base else c.base
    P, mP, LP = ops.calc_pn(*_pn_args(c), parent_log2p=dv(base))
    torch.cuda.synchronize()
    return host(P), host(mP), host(LP)


# ------------------------------------------------------------------------------------------------------------ tn_calc_pn
@pytest.mark.parametrize('name', list(bk.PN_CASES))
def test_calc_pn_against_reference(name):
    """P and minP of every branch within 2 x tol of pn_table_ref; all-zero tables exactly 1/q with flag exactly -1; the exact-arithmetic
    cases bit for bit (entries equal to |min| are not lifted and not counted).
    Worst error / tol measured on an MI355X: 0.19 ('stride257'); 0.02 .. 0.15 on the other cases (printed per case)."""
    c = bk.pn_case(name)
    P, mP, _ = _calc(name)
    worst = 0.0
    for k, (want, ref) in enumerate(zip(c.regimes, bk.pn_case_refs(name))):
        rP, rm = bk.pn_error_ratios(ref, P[k], mP[k])
        worst = max(worst, rP, rm)
        assert rP <= 2.0 and rm <= 2.0, (name, k, want, rP, rm)
        if want == 'zero':
            assert np.all(P[k] == 1.0 / ref.q) and mP[k] == -1.0
        if c.exact:
            assert same_bits(P[k], ref.P) and mP[k] == ref.minP == -0.25
    print('calc_pn %s: worst error / tol %.3f' % (name, worst))


@pytest.mark.parametrize('name', list(bk.PN_CASES))
def test_calc_pn_log2p(name):
    """log2p_out is -inf exactly where P == 0 and everywhere under a -inf parent, never NaN; elsewhere it lies within 2 x LOG2P_MAX_ULPS
    of the correctly rounded log2(P) + parent of the device's own P (a strided sample of every branch).
    Largest distance measured on an MI355X over all cases: 1 ulp (LOG2P_MAX_ULPS; 0 on the smallest tables), so 2 ulp are asserted."""
    c = bk.pn_case(name)
    P, _, LP = _calc(name)
    assert not np.isnan(LP).any()
    worst = 0.0
    for k in range(len(c.branches)):
        if c.base[k] == -math.inf:
            assert np.all(LP[k] == -math.inf)
            continue
        assert np.array_equal(LP[k] == -math.inf, P[k] == 0.0) and np.all(LP[k] <= c.base[k])
        sel = np.unique(np.concatenate([np.arange(0, P[k].size, max(1, P[k].size // ULP_SAMPLE)), [P[k].size - 1]]))
        sel = sel[P[k][sel] > 0]
        if sel.size:
            worst = max(worst, float(bk.ulps(LP[k][sel], bk.log2p_ref(P[k][sel], c.base[k])).max()))
    print('calc_pn %s: log2p_out at most %.3f ulp from the correctly rounded value' % (name, worst))
    assert worst <= 2.0 * LOG2P_MAX_ULPS


def test_calc_pn_refused_above_150k_writes_nothing(L):
    """One state more than fits 150 KiB of LDS: -1, and P, minP and log2p_out keep every byte."""
    c = bk.pn_case('refused_calc')
    q, p, Dr, br, nl, nu = c.shape
    nb = len(c.branches)
    a = _pn_args(c)
    base = dv(c.base)
    P, mP, LP = Guarded.of(F64, (nb, q), SENT), Guarded.of(F64, (nb,), SENT), Guarded.of(F64, (nb, q), SENT)
    rc = L.tn_calc_pn(*[t.data_ptr() for t in a], nb, q, nl, nu, p, Dr, br, P.ptr, mP.ptr, base.data_ptr(), LP.ptr, _st())
    torch.cuda.synchronize()
    assert rc == -1 and 'calc_pn' in _msg(L)
    for g in (P, mP, LP):
        assert g.untouched(SENT) and g.intact()


def test_calc_pn_nan_row():
    """A NaN in one row d of one prefix's T1: the branches of that prefix return NaN for the states with dmap[s] = d and the flag -1;
    every other branch is unchanged bit for bit."""
    from tnac4o_amd import ops
    c = bk.pn_case('stride256')
    d = 2
    T1 = c.T1.copy()
    T1[1, d, 3] = np.nan
    P, mP, LP = (host(x) for x in ops.calc_pn(*_pn_args(c, T1), parent_log2p=dv(c.base)))
    P0, mP0, LP0 = _calc('stride256')
    hit = c.branches[:, 0] == 1
    assert 0 < hit.sum() < len(hit) and np.any(c.dmap == d)
    for k in range(len(hit)):
        if hit[k]:
            assert np.all(np.isnan(P[k][c.dmap == d])) and mP[k] == -1.0
        else:
            assert same_bits(P[k], P0[k]) and same_bits(mP[k:k + 1], mP0[k:k + 1]) and same_bits(LP[k], LP0[k])


# ------------------------------------------------------------------------------------------------------------ tn_sample_pn / tn_score_pn
def _groups(c, seed):
    """Members of the groups (one group per branch of the case): sample indices in any order."""
    rng = np.random.default_rng([90, seed])
    ng = len(c.branches)
    sizes = [GROUP_SIZES[g % len(GROUP_SIZES)] for g in range(ng)]
    n = int(np.sum(sizes))
    return rng, rng.permutation(n).astype(np.int32), np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), n


@pytest.mark.parametrize('name', SCORE_CASES)
def test_score_pn_same_bits_as_calc_pn(name):
    """The flag and the increments of tn_score_pn are tn_calc_pn's bits at the workload shape, at chi = 128, on both sides of the 48 KiB
    and 64 KiB crossings of the dynamic LDS and at the 150 KiB limit."""
    from tnac4o_amd import ops
    c = bk.pn_case(name)
    q = c.shape[0]
    P, mP, LP = _calc(name, True)
    rng, perm, starts, n = _groups(c, 1)
    forced = rng.integers(0, q, (n, 3)).astype(np.int16)
    forced[perm[starts[:-1]], 1] = q - 1                         # the last state, once per group
    child, log2p, mP2, cells = ops.score_pn(*_pn_args(c), dv(perm), dv(starts), dv(forced), 1, cells=True)
    child, log2p, mP2, cells = host(child), host(log2p), host(mP2), host(cells)
    assert same_bits(mP2, mP)
    assert np.array_equal(child, forced[:, 1]) and not cells[:, 0].any() and not cells[:, 2].any()
    for g in range(len(c.branches)):
        mem = perm[starts[g]:starts[g + 1]]
        assert same_bits(log2p[mem], LP[g][forced[mem, 1]]) and same_bits(cells[mem, 1], log2p[mem]), (name, g)


@pytest.mark.parametrize('name', SAMPLE_CASES)
def test_sample_pn_same_bits_as_calc_pn(name):
    """The flag and the increments of tn_sample_pn are tn_calc_pn's bits at the workload shape, at chi = 128, on both sides of the
    kernel's own 48 KiB crossing ((max(front, q) + q) * 8) and at its 150 KiB limit; the draws follow numpy on the table (draws within
    1e-9 of a running sum are left out, at most 1 %, as tests/test_gpu_sampling.py::test_sample_pn_against_numpy does)."""
    from tnac4o_amd import ops
    c = bk.pn_case(name)
    q = c.shape[0]
    P, mP, LP = _calc(name, True)
    rng, perm, starts, n = _groups(c, 2)
    r = rng.random(n)
    child, log2p, mP2 = (host(x) for x in ops.sample_pn(*_pn_args(c), dv(perm), dv(starts), dv(r)))
    assert same_bits(mP2, mP) and np.all((child >= 0) & (child < q))
    left_out = 0
    for g in range(len(c.branches)):
        mem = perm[starts[g]:starts[g + 1]]
        assert np.all(P[g][child[mem]] > 0) and same_bits(log2p[mem], LP[g][child[mem]]), (name, g)
        for k in mem:
            if sref.boundary_distance(P[g], r[k]) < 1e-9:
                left_out += 1
                continue
            assert child[k] == sref.draw_np(P[g], r[k]), (name, g, k, r[k])
    assert left_out <= 0.01 * n


def _group_ptrs(c, kind):
    ng = len(c.branches)
    rng, perm, starts, n = _groups(c, 3)
    keep = _pn_args(c) + [dv(perm), dv(starts)]
    child, log2p, mP = Guarded.of(torch.int32, (n,), SENT), Guarded.of(F64, (n,), SENT), Guarded.of(F64, (ng,), SENT)
    return keep, ng, n, rng, child, log2p, mP


def test_sample_pn_refused_above_150k_writes_nothing(L):
    c = bk.pn_case('refused_sample')
    q, p, Dr, br, nl, nu = c.shape
    keep, ng, n, rng, child, log2p, mP = _group_ptrs(c, 'sample')
    r = dv(rng.random(n))
    rc = L.tn_sample_pn(*[t.data_ptr() for t in keep], ng, r.data_ptr(), q, nl, nu, p, Dr, br, child.ptr, log2p.ptr, mP.ptr, _st())
    torch.cuda.synchronize()
    assert rc == -1 and 'sample_pn' in _msg(L)
    for g in (child, log2p, mP):
        assert g.untouched(SENT) and g.intact()


def test_score_pn_refused_above_150k_writes_nothing(L):
    c = bk.pn_case('refused_calc')
    q, p, Dr, br, nl, nu = c.shape
    keep, ng, n, rng, child, log2p, mP = _group_ptrs(c, 'score')
    forced = dv(rng.integers(0, q, (n, 2)).astype(np.int16))
    cells = Guarded.of(F64, (n, 2), SENT)
    rc = L.tn_score_pn(*[t.data_ptr() for t in keep], ng, forced.data_ptr(), 2, 0, q, nl, nu, p, Dr, br, child.ptr, log2p.ptr, cells.ptr, mP.ptr,
                       _st())
    torch.cuda.synchronize()
    assert rc == -1 and 'score_pn' in _msg(L)
    for g in (child, log2p, mP, cells):
        assert g.untouched(SENT) and g.intact()


# ------------------------------------------------------------------------------------------------------------ tn_env_rr_batched
@pytest.mark.parametrize('name', list(bk.ENV_RR_CASES))
def test_env_rr_against_exact(name):
    """Every returned block is the exact contraction times the exact power of two (largest magnitude in [1, 2)), within 2 x the bound
    (Dr + br + 2) u sum |A| |RR| |W|; the zero parent comes back as zeros.  Shapes with more than 1024 outputs (accumulator slots 4..7),
    a partly used last slot, and 64 KiB / 96 KiB / 150 KiB of dynamic LDS.
    Worst error / bound measured on an MI355X: 0.41 ('slot5'), 0.02 .. 0.06 on the other shapes."""
    from tnac4o_amd import ops
    c = bk.env_rr_case(name)
    out = host(ops.env_rr(dv(c.A), dv(c.RRp), dv(c.W), dv(c.parent), dv(c.uidx)))
    assert out.shape == (3, c.shape[0], c.shape[3])
    worst = 0.0
    for k, ref in enumerate(bk.env_rr_case_refs(name)):
        assert ref.ambiguous == 0
        r = bk.env_rr_error_ratio(ref, out[k])
        worst = max(worst, r)
        assert r <= 2.0, (name, k, r)
        m = np.abs(out[k]).max()
        assert (m == 0.0 and not out[k].any()) if ref.expo is None else 1.0 <= m < 2.0
    print('env_rr %s: worst error / bound %.4f' % (name, worst))


@pytest.mark.parametrize('name', list(bk.ENV_RR_REFUSED))
def test_env_rr_refused_writes_nothing(L, name):
    """One physical index more than fits 150 KiB of LDS, and Dl * bl = 2049: -1, and the output keeps every byte."""
    c = bk.env_rr_case(name)
    Dl, p, Dr, bl, br, pu = c.shape
    keep = [dv(c.A), dv(c.RRp), dv(c.W), dv(c.parent), dv(c.uidx)]
    out = Guarded.of(F64, (3, Dl, bl), SENT)
    rc = L.tn_env_rr_batched(*[t.data_ptr() for t in keep], 3, Dl, p, Dr, bl, br, pu, out.ptr, _st())
    torch.cuda.synchronize()
    assert rc == -1 and 'env_rr' in _msg(L)
    assert out.untouched(SENT) and out.intact()


# ------------------------------------------------------------------------------------------------------------ tn_env_rl_batched
@pytest.mark.parametrize('Dr', bk.ENV_RL_DR)
@pytest.mark.parametrize('nk', bk.ENV_RL_NK)
def test_env_rl_bit_for_bit(L, Dr, nk):
    """Rows shorter than, equal to and longer than a wave, key counts that leave the last workgroup partly filled; a zero row, a
    subnormal row and the last row of T1; nothing written past the nk rows."""
    for first in range(3 if nk < 3 else 1):
        T1, par, didx = bk.env_rl_case(Dr, nk, first)
        keep = [dv(T1), dv(par), dv(didx)]
        out = Guarded.of(F64, (nk, Dr))
        assert L.tn_env_rl_batched(*[t.data_ptr() for t in keep], nk, T1.shape[1], Dr, out.ptr, _st()) == 0, _msg(L)
        torch.cuda.synchronize()
        assert out.intact() and same_bits(out.host(), bk.env_rl_ref(T1, par, didx)), (Dr, nk, first)


# ------------------------------------------------------------------------------------------------------------ tn_merge_groups
def _merge_run(c):
    """The kernel on a case, every member array one element longer than the members (the extra element would win every comparison), so
    that a read at starts[ng] stays inside the tensors."""
    from tnac4o_amd import ops
    E, lp = np.append(c.E, -1e300), np.append(c.lp, 12345.0)
    deg, pos = np.append(c.deg, 999), np.append(c.pos, 424242)
    rep, dn, ln = ops.merge_groups(dv(E), dv(lp), dv(deg), dv(pos), dv(c.starts), c.min_dEng)
    torch.cuda.synchronize()
    return host(rep), host(dn), host(ln)


@pytest.mark.parametrize('name', [n for n in bk.MERGE_CASES if n not in bk.MERGE_EMPTY])
def test_merge_groups_bit_for_bit(name):
    """One, 255 .. 257 and 70001 groups of 1 to 1000 members: the first member of minimal energy under ties, the window's '<=' at
    min_dEng = 0 and at a member exactly on the edge, a lone representative's own log2p (-0.0 kept), -inf members, degeneracies that add
    up past 2^62."""
    c = bk.merge_case(name)
    rep, dn, ln = _merge_run(c)
    r_rep, r_dn, r_ln = bk.merge_groups_ref(c.E, c.lp, c.deg, c.pos, c.starts, c.min_dEng)
    assert np.array_equal(rep, r_rep) and np.array_equal(dn, r_dn) and same_bits(ln, r_ln)


@pytest.mark.parametrize('name', bk.MERGE_EMPTY)
def test_merge_groups_empty_groups(name):
    """Empty groups, alone, in the middle and at the end, in one and in several blocks: rep_pos = -1, deg = 0, log2p = -inf, without a
    read of the members (the element after the last member would otherwise come back as the last group's representative)."""
    c = bk.merge_case(name)
    rep, dn, ln = _merge_run(c)
    r_rep, r_dn, r_ln = bk.merge_groups_ref(c.E, c.lp, c.deg, c.pos, c.starts, c.min_dEng)
    empty = np.diff(c.starts) == 0
    assert empty[-1] and rep[-1] == -1 and dn[-1] == 0 and ln[-1] == -math.inf
    assert np.array_equal(rep, r_rep) and np.array_equal(dn, r_dn) and same_bits(ln, r_ln)
    assert np.all(rep[empty] == -1) and np.all(rep[~empty] != -1)


# ------------------------------------------------------------------------------------------------------------ tn_nfactor_batched
@pytest.mark.parametrize('n', bk.NFACTOR_LEN)
@pytest.mark.parametrize('batch', (1, 3))
def test_nfactor_batched_bit_for_bit(L, n, batch):
    """Blocks of 1, 255 .. 257 and 70000 doubles, alone and three to a call: a zero block stays zero, a subnormal block is multiplied
    by 2^1023, a graded block by the inverse of its exact power of two; nothing written past the blocks."""
    sets = [[k] for k in bk.NFACTOR_KINDS] if batch == 1 else [list(bk.NFACTOR_KINDS), list(bk.NFACTOR_KINDS[::-1])]
    for kinds in sets:
        X = np.stack([bk.nfactor_block(k, n, j) for j, k in enumerate(kinds)])
        x = Guarded.of(F64, X.shape)
        x.tensor().copy_(dv(X))
        assert L.tn_nfactor_batched(x.ptr, len(kinds), n, _st()) == 0, _msg(L)
        torch.cuda.synchronize()
        assert x.intact() and same_bits(x.host(), bk.nfactor_batched_ref(X)), (n, kinds)
