"""CPU checks of the sampling surface (tnac4o.sample_boltzmann): the log2 Z estimators, layout and validation of the uniform numbers,
the chunk planner, the exact log2 Z references against each other and against the oracle's forced walk, and the argument errors of
tn_sample_pn / tn_gibbs_sample (no launch, no GPU needed)."""
import ctypes

import numpy as np
import pytest

import sampling_ref as sref
from oracle import solver_ref as sr
from tnac4o_amd import auxx, sampler
from tnac4o_amd.beam import _Cell


# ---------------------------------------------------------------------------------------------- estimators
def test_estimators_definitions():
    rng = np.random.default_rng(3)
    for centre in (-1000.0, 0.0, 1000.0):
        s = centre + rng.normal(0.0, 2.0, 200)
        beta = 1.7
        lq = rng.uniform(-30.0, -1.0, 200)
        E = -(s + lq) * sampler.LN2 / beta
        got, lower, est = sampler.log2z_estimators(E, lq, beta)
        np.testing.assert_allclose(got, s, rtol=0, atol=1e-9)
        assert lower == pytest.approx(float(np.mean(got)), abs=1e-12)
        ref = float(np.log2(np.mean(np.exp2(got - centre)))) + centre      # a shift other than the maximum
        assert est == pytest.approx(ref, abs=1e-9)
        assert np.isfinite(est) and lower <= est


def test_estimators_coincide_for_equal_samples_and_one_sample():
    for v in (-1000.0, 916.3453, 1000.0):
        lq = np.full(17, -12.5)
        E = -(v + lq) * sampler.LN2 / 3.0
        s, lower, est = sampler.log2z_estimators(E, lq, 3.0)
        assert np.all(np.abs(s - v) <= 1e-9)
        assert abs(lower - est) <= 1e-12 and lower <= est
        s1, l1, e1 = sampler.log2z_estimators(E[:1], lq[:1], 3.0)
        assert s1.shape == (1,) and l1 == s1[0] and e1 == s1[0]


def test_estimators_mean_below_estimate_always():
    rng = np.random.default_rng(8)
    for t in range(200):
        n = int(rng.integers(1, 40))
        E = rng.normal(0.0, 10.0 ** rng.integers(-3, 3), n)
        lq = -rng.uniform(0.0, 50.0, n)
        _, lower, est = sampler.log2z_estimators(E, lq, float(rng.uniform(0.1, 5.0)))
        assert lower <= est


def test_estimators_reject_bad_shapes():
    with pytest.raises(ValueError):
        sampler.log2z_estimators(np.zeros(0), np.zeros(0), 1.0)
    with pytest.raises(ValueError):
        sampler.log2z_estimators(np.zeros((2, 2)), np.zeros((2, 2)), 1.0)


# ---------------------------------------------------------------------------------------------- uniform numbers
def test_default_uniforms_consume_the_stream_like_one_rand_per_cell():
    np.random.seed(77)
    u = sampler.check_uniforms(None, 6, 11)
    np.random.seed(77)
    ref = np.stack([np.random.rand(11) for _ in range(6)])
    assert u.shape == (6, 11) and u.dtype == np.float64 and np.array_equal(u, ref)


def test_uniforms_validation():
    good = np.random.default_rng(0).random((6, 5))
    assert sampler.check_uniforms(good, 6, 5) is good
    bad = [good.T.copy(), good[:, :4], good.reshape(-1), good.astype(np.float32), [[0.5] * 5] * 6, 'x']
    for name, v in (('one', 1.0), ('neg', -1e-300), ('nan', np.nan), ('inf', np.inf)):
        b = good.copy()
        b[3, 2] = v
        bad.append(b)
    for b in bad:
        with pytest.raises(ValueError):
            sampler.check_uniforms(b, 6, 5)
    edge = good.copy()
    edge[0, 0], edge[5, 4] = 0.0, np.nextafter(1.0, 0.0)
    assert sampler.check_uniforms(edge, 6, 5) is edge
    import torch
    t = torch.as_tensor(good)
    assert sampler.check_uniforms(t, 6, 5) is t
    with pytest.raises(ValueError):
        sampler.check_uniforms(t.to(torch.float32), 6, 5)
    with pytest.raises(ValueError):
        sampler.check_uniforms(t + 1.0, 6, 5)


def test_sample_boltzmann_rejects_bad_input_before_any_device_work():
    """The validation runs before the boundaries are built: the solver is never asked for rhoT."""
    import tnac4o_amd
    ins = tnac4o_amd.tnac4o(mode='RMF', Nx=3, Ny=3, J=auxx.synthetic_rmf(3, 3, 3, 17), beta=1.0)

    def boom(**kw):
        raise AssertionError('device work before validation')
    ins._setup_rhoT = boom
    with pytest.raises(ValueError):
        ins.sample_boltzmann(M=4, uniforms=np.zeros((9, 5)))
    with pytest.raises(ValueError):
        ins.sample_boltzmann(M=4, uniforms=np.full((9, 4), 1.0))
    with pytest.raises(ValueError):
        ins.sample_boltzmann(M=0)
    with pytest.raises(ValueError):
        ins.sample_boltzmann(M=4, chunk=0)
    with pytest.raises(ValueError):
        ins.sample_boltzmann(M=4, chunk=2.5)


# ---------------------------------------------------------------------------------------------- chunks
def test_chunk_planner():
    ws = lambda m: 1000 + 10 * m
    assert sampler.plan_chunk(1000, ws, 10 ** 9) == 512                  # the largest power of two <= M
    assert sampler.plan_chunk(1024, ws, 10 ** 9) == 1024
    assert sampler.plan_chunk(1, ws, 10 ** 9) == 1
    assert sampler.plan_chunk(1 << 20, ws, 1000 + 10 * 300) == 256       # the budget decides
    assert sampler.plan_chunk(1 << 20, ws, 1010) == 1
    with pytest.raises(MemoryError):
        sampler.plan_chunk(16, ws, 1009)
    assert sampler.plan_chunk(1 << 30, ws, 10 ** 12, B=1 << 10) == 1 << 21      # chunk^2 B^2 < 2^63
    with pytest.raises(ValueError):
        sampler.plan_chunk(0, ws, 10 ** 9)


def test_chunk_slices_cover_in_order():
    assert sampler.chunk_slices(10, 4) == [(0, 4), (4, 8), (8, 10)]
    assert sampler.chunk_slices(8, 8) == [(0, 8)]
    assert sampler.chunk_slices(3, 100) == [(0, 3)]
    for bad in (0, -1, 1.5, None):
        with pytest.raises(ValueError):
            sampler.chunk_slices(8, bad)


def test_cell_misfit_names_the_lds_bound():
    assert sampler.cell_misfit(256, 16, 32, 16) is None
    assert sampler.cell_misfit(9600, 2, 2, 2) is None
    assert 'LDS' in sampler.cell_misfit(9601, 2, 2, 2)
    assert 'LDS' in sampler.cell_misfit(256, 64, 512, 64)


# ---------------------------------------------------------------------------------------------- draw rule
def test_draw_rule():
    P = np.array([0.0, 0.25, 0.0, 0.5, 0.25, 0.0])
    assert sref.draw_np(P, 0.0) == 1                  # r = 0 lands on the zero entry 0: forward
    assert sref.draw_np(P, 0.1) == 1
    assert sref.draw_np(P, 0.25) == 1                 # side 'left': a running sum equal to r is taken
    assert sref.draw_np(P, np.nextafter(0.25, 1)) == 3
    assert sref.draw_np(P, 0.75) == 3
    assert sref.draw_np(P, 0.9) == 4
    assert sref.draw_np(P, np.nextafter(1.0, 0.0)) == 4
    assert sref.draw_np(P, 1.5) == 4                  # above the last running sum: the last positive entry
    assert sref.draw_np(np.array([1.0]), 0.3) == 0
    Q = np.full(10, 0.1)                              # the running sum ends below 1 in floating point or not: never out of range
    assert sref.draw_np(Q, np.nextafter(1.0, 0.0)) == 9


# ---------------------------------------------------------------------------------------------- exact log2 Z
def test_exact_log2Z_references():
    """The chimera ring against the values recorded with the feature request; the RMF enumeration against the plain sum taken in the
    opposite order."""
    want = {0.5: 38.482315042469, 1.0: 54.803873696243, 3.0: 142.760031518249}
    for beta, v in want.items():
        assert sref.exact_log2Z('chimera2x2', beta) == pytest.approx(v, abs=1e-9)
    J = auxx.synthetic_rmf(3, 3, 3, 17)
    import itertools
    states = np.array(list(itertools.product(range(3), repeat=9)), dtype=np.int64)[::-1]
    for beta in (0.5, 1.0, 3.0):
        z = np.sum(np.exp(-beta * auxx.energy_RMF(J, states)))
        assert sref.exact_log2Z('rmf3x3', beta) == pytest.approx(float(np.log2(z)), abs=1e-11)


@pytest.mark.parametrize('beta', [0.5, 1.0, 3.0])
@pytest.mark.parametrize('case', ['ising3x3', 'rmf3x3'])
def test_oracle_forced_walk_gives_exact_log2Z(case, beta):
    """For an exact contraction -beta E / ln 2 - log2 q(x) = log2 Z for EVERY configuration x: the oracle's walk forced along random
    configurations against the enumeration (for the Ising instance: after the 1 of its spin without any term).  The identity holds to
    3e-14 on these instances; 1e-12 leaves room for the platform's BLAS."""
    rng = np.random.default_rng(5)
    if case == 'rmf3x3':
        J = auxx.synthetic_rmf(3, 3, 3, 17)
        ref = sr.RefSolver(mode='RMF', Nx=3, Ny=3, J=J, beta=beta)
        states = rng.integers(0, 3, (12, 9))
    else:
        import marginals_ref as mr
        ref = sr.RefSolver(mode='Ising', Nx=3, Ny=3, Nc=2, J=mr.ising_3x3_nc2(), beta=beta)
        states = np.stack([rng.integers(0, int(ref.N[k // 3][k % 3]), 12) for k in range(9)], axis=1)
    lq, Pc = sref.oracle_log2q(ref, states, Dmax=64, tolS=1e-15)
    assert Pc.shape == (12, 9) and np.all(Pc > 0) and np.all(Pc <= 1)
    ref.states = states[:, ref.order]
    if case == 'rmf3x3':
        E = auxx.energy_RMF(J, ref.states)
    else:
        E = sr.energy_Jij(mr.ising_3x3_nc2(), ref.binary_states())
    s, lower, est = sampler.log2z_estimators(E, lq, beta)
    exact = sref.exact_log2Z(case, beta)
    assert float(np.max(np.abs(s - exact))) <= 1e-12, (s - exact)
    assert abs(lower - exact) <= 1e-12 and abs(est - exact) <= 1e-12


# ---------------------------------------------------------------------------------------------- argument errors of the exports
def _lib():
    from tnac4o_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _msg(L):
    buf = ctypes.create_string_buffer(256)
    L.tn_last_error(buf, 256)
    return buf.value.decode()


def _expect_neg(L, rc, text):
    assert rc < 0, rc
    assert text in _msg(L), _msg(L)


def test_sample_pn_argument_errors():
    L = _lib()
    host = (ctypes.c_double * 64)()
    P = ctypes.cast(host, ctypes.c_void_p)               # a host address standing in for device memory: never dereferenced

    def sp(T1=P, perm=P, starts=P, uni=P, child=P, lq=P, mp=P, ng=4, q=16, nl=1, nu=1, p=1, Dr=1, br=1):
        return L.tn_sample_pn(T1, P, P, P, P, P, P, P, P, perm, starts, ng, uni, q, nl, nu, p, Dr, br, child, lq, mp, None)
    for kw in ({'T1': None}, {'perm': None}, {'starts': None}, {'uni': None}, {'child': None}, {'lq': None}, {'mp': None}):
        _expect_neg(L, sp(**kw), 'null operand')
    _expect_neg(L, sp(ng=-1), 'negative group count')
    _expect_neg(L, sp(q=0), 'non-positive dimension')
    _expect_neg(L, sp(br=0), 'non-positive dimension')
    _expect_neg(L, sp(q=256, p=64, Dr=512, br=64), 'LDS')                # the environments alone are too large (tn_calc_pn's bound)
    _expect_neg(L, sp(q=9601, p=2, Dr=2, br=2), 'LDS')                   # fits tn_calc_pn, not table + running sum
    assert sp(q=9600, p=2, Dr=2, br=2, ng=0) == 0
    assert sp(ng=0) == 0                                                 # nothing to do: no launch


def test_gibbs_sample_argument_errors():
    L = _lib()
    host = (ctypes.c_double * 64)()
    P = ctypes.cast(host, ctypes.c_void_p)
    cells = (_Cell * 1)()
    c = cells[0]
    for n in ('F', 'dmap', 'rmap', 'down', 'right', 'Es', 'A'):
        setattr(c, n, P.value)
    c.q, c.nl, c.nu, c.pd, c.br, c.e1cols, c.e4cols, c.Dl, c.p, c.Dr = 4, 1, 1, 2, 1, 1, 1, 1, 2, 2
    gmin, mg = ctypes.c_double(0.0), ctypes.c_int64(0)
    big = 1 << 40

    def gs(cl=cells, M=8, B=4, uni=P, ldu=8, st=P, E=P, lq=P, gm=ctypes.byref(gmin), ws=P, wsb=big):
        return L.tn_gibbs_sample(1, 1, ctypes.cast(cl, ctypes.c_void_p) if cl is not None else None, M, B, uni, ldu, st, E, lq, gm,
                                 ctypes.byref(mg), ws, wsb, None)
    assert L.tn_gibbs_sample_ws_bytes(4, 4, 64, 256, 64, 64, 256) > 0
    # the query does not grow with q: no table is ever materialised
    assert L.tn_gibbs_sample_ws_bytes(4, 4, 64, 256, 64, 64, 256) == L.tn_gibbs_sample_ws_bytes(4, 4, 64, 4, 64, 64, 256)
    _expect_neg(L, gs(cl=None), 'bad arguments')
    _expect_neg(L, gs(M=0), 'bad arguments')
    _expect_neg(L, gs(B=0), 'bad arguments')
    _expect_neg(L, gs(ws=None), 'bad arguments')
    _expect_neg(L, gs(M=1 << 31), 'too many samples')
    _expect_neg(L, gs(uni=None), 'uniforms')
    _expect_neg(L, gs(ldu=7), 'uniforms')
    for kw in ({'st': None}, {'E': None}, {'lq': None}, {'gm': None}):
        _expect_neg(L, gs(**kw), 'null result pointer')
    _expect_neg(L, gs(M=1 << 20, B=1 << 12, ldu=1 << 20), 'exceeds int64')
    need = L.tn_gibbs_sample_ws_bytes(1, 1, 8, 4, 2, 4, 2)
    rc = gs(wsb=need - 8)
    assert rc == -3
    _expect_neg(L, rc, 'workspace too small')
    c.q = 40000
    _expect_neg(L, gs(), 'bad cell')
    c.q, c.p = 4, 3
    _expect_neg(L, gs(), 'vertical bond')
    c.p, c.Dl, c.nl = 2, 1025, 2
    _expect_neg(L, gs(), '2048')
    c.Dl, c.nl, c.q = 1, 1, 9700
    _expect_neg(L, gs(), 'LDS')
