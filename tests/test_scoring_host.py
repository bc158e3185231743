"""Host logic of tnac4o.calculate_log_probability and tnac4o.calculate_free_energy (no GPU): the round trip between spin read-outs and
cell states, the validation of the configurations to score, the assembly of log2 Z from row contractions and overlaps, and the
argument errors both calls and the exports tn_score_pn / tn_gibbs_score raise before any device work."""
import ctypes

import numpy as np
import pytest

import marginals_ref as mr
from tnac4o_amd import auxx, sampler
from tnac4o_amd.beam import _Cell

LN2 = float(np.log(2.0))


def ising(beta=1.0):
    import tnac4o_amd
    return tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=mr.ising_3x3_nc2(), beta=beta)


def rmf(beta=1.0):
    import tnac4o_amd
    return tnac4o_amd.tnac4o(mode='RMF', Nx=3, Ny=3, J=auxx.synthetic_rmf(3, 3, 3, 17), beta=beta)


# ---------------------------------------------------------------------------------------------- states_from_binary
@pytest.mark.parametrize('rot', [0, 1, 3])
def test_states_from_binary_round_trip(rot):
    """ising_3x3_nc2 has an inactive spin (9, in cell 4): that cell has two states, every other cell four."""
    ins = ising()
    if rot:
        ins.rotate_graph(rot)
    q = np.array([4, 4, 4, 4, 2, 4, 4, 4, 4])
    rng = np.random.default_rng(3 + rot)
    st = rng.integers(0, q[None, :], size=(200, 9))
    ins.states = st.astype(ins.indtype)
    bits = ins.binary_states()
    assert bits.shape == (200, 18) and np.all(bits[:, 9] == 2) and set(np.unique(np.delete(bits, 9, axis=1))) == {0, 1}
    back = ins.states_from_binary(bits)
    assert back.dtype == np.int64 and np.array_equal(back, st)
    # the entry of the inactive spin is ignored, whatever it holds
    for junk in (0, 1, 7):
        b2 = bits.copy()
        b2[:, 9] = junk
        assert np.array_equal(ins.states_from_binary(b2), st)
    # 1 is up: all spins up is state 0 of every cell, all down the last state
    assert np.array_equal(ins.states_from_binary(np.ones((1, 18), dtype=np.int8))[0], np.zeros(9))
    assert np.array_equal(ins.states_from_binary(np.zeros((1, 18), dtype=np.int8))[0], q - 1)
    # and the other way round
    ins.states = back
    assert np.array_equal(ins.binary_states(), bits)


def test_states_from_binary_errors():
    ins = ising()
    with pytest.raises(ValueError):
        ins.states_from_binary(np.zeros((4, 17), dtype=np.int8))
    with pytest.raises(ValueError):
        ins.states_from_binary(np.zeros(18, dtype=np.int8))
    with pytest.raises(ValueError):
        ins.states_from_binary(np.zeros((4, 18)))
    bad = np.ones((2, 18), dtype=np.int8)
    bad[1, 3] = 2
    with pytest.raises(ValueError):
        ins.states_from_binary(bad)
    with pytest.raises(ValueError):
        rmf().states_from_binary(np.zeros((1, 9), dtype=np.int8))


# ---------------------------------------------------------------------------------------------- check_states
def test_check_states():
    q = np.array([3, 256, 2])
    st = np.array([[2, 255, 1], [0, 0, 0]])
    out = sampler.check_states(st, q)
    assert out.dtype == np.int64 and np.array_equal(out, st)
    # the solver's own int8 storage of 256 states reads as unsigned
    assert np.array_equal(sampler.check_states(st.astype(np.int8), q), st)
    assert np.array_equal(sampler.check_states(st.astype(np.uint16), q), st)
    for bad in (st.astype(np.float64), st[0], st[:, :2], st[:0], st.tolist(), st.astype(bool), None):
        with pytest.raises(ValueError):
            sampler.check_states(bad, q)
    for m, k, v in ((0, 0, 3), (1, 1, 256), (1, 2, 2), (0, 0, -1)):
        b = st.copy()
        b[m, k] = v
        with pytest.raises(ValueError, match='outside'):
            sampler.check_states(b, q)
    b = st.astype(np.int8)
    b[0, 0] = -1                                         # reads as 255: outside a cell of 3 states
    with pytest.raises(ValueError, match='outside'):
        sampler.check_states(b, q)


def test_cell_misfit_without_running_sum():
    """tn_score_pn holds tn_calc_pn's bound: a table that does not fit next to its running sum may still be scored."""
    assert sampler.cell_misfit(9601, 2, 2, 2) is not None
    assert sampler.cell_misfit(9601, 2, 2, 2, running_sum=False) is None
    assert sampler.cell_misfit(19188, 2, 2, 2, running_sum=False) is None            # (12 + 19188) * 8 = 150 KiB exactly
    assert 'tn_score_pn' in sampler.cell_misfit(19189, 2, 2, 2, running_sum=False)
    assert sampler.cell_misfit(256, 64, 512, 64, running_sum=False) is not None


# ---------------------------------------------------------------------------------------------- assembly of log2 Z
def test_log2z_from_rows():
    """Z = prod r / prod o with every interior boundary scaled by an arbitrary factor of either sign: rows and overlaps move, the
    result does not."""
    rng = np.random.default_rng(8)
    Ny, beta = 5, 0.7
    Z = 3.5e7
    b = np.concatenate([[1.0], rng.uniform(0.1, 9.0, Ny - 1) * rng.choice([-1.0, 1.0], Ny - 1)])      # b_0 = 1
    t = np.concatenate([rng.uniform(0.1, 9.0, Ny - 1) * rng.choice([-1.0, 1.0], Ny - 1), [1.0]])      # t_1 .. t_Ny, t_Ny = 1
    assert (b < 0).any() and (t < 0).any()
    r = Z / (b * t)                                       # Z = b_ny t_{ny+1} r_ny
    o = Z / (b[1:] * t[:-1])                              # Z = b_ny t_ny o_ny
    assert (r < 0).any() and (o < 0).any()
    shifts = rng.normal(0.0, 2.0, (Ny * 3, 3))
    want = np.log2(Z) - beta / LN2 * shifts.sum()
    got, lr, lo = sampler.log2z_from_rows(r, o, shifts, beta)
    assert abs(got - want) <= 1e-12 * abs(want)
    assert np.allclose(lr, np.log2(np.abs(r)), rtol=0, atol=1e-13) and np.allclose(lo, np.log2(np.abs(o)), rtol=0, atol=1e-13)
    # mantissa and power-of-two exponent apart: the same number, also where the product would leave the double range
    er, eo = rng.integers(-2000, 2000, Ny), rng.integers(-2000, 2000, Ny - 1)
    got2, lr2, lo2 = sampler.log2z_from_rows(r, o, shifts, beta, rows_log2=er, overlaps_log2=eo)
    assert abs(got2 - (want + er.sum() - eo.sum())) <= 1e-12 * max(abs(want), float(np.abs(er).sum()))
    assert np.allclose(lr2 - lr, er, rtol=0, atol=1e-12) and np.allclose(lo2 - lo, eo, rtol=0, atol=1e-12)
    # trivial ends that are not 1 are divided out; a single row needs no overlap
    got3, _, _ = sampler.log2z_from_rows(r, o, shifts, beta, ends=(-2.0, 0.25))
    assert abs(got3 - (want + 1.0)) <= 1e-12 * abs(want)
    one, lr1, lo1 = sampler.log2z_from_rows([8.0], [], 0.0, 1.0)
    assert one == 3.0 and lr1.shape == (1,) and lo1.shape == (0,)
    for bad in (([1.0, 2.0], [1.0, 1.0]), ([], []), ([1.0], [1.0])):
        with pytest.raises(ValueError):
            sampler.log2z_from_rows(bad[0], bad[1], 0.0, 1.0)
    with pytest.raises(ValueError):
        sampler.log2z_from_rows(r, o, shifts, beta, rows_log2=er[:-1])


# ---------------------------------------------------------------------------------------------- argument errors of the calls
@pytest.mark.parametrize('make', [ising, rmf])
def test_calculate_log_probability_validates_before_any_device_work(make):
    ins = make()
    ins.rotate_graph(1)
    ok = np.zeros((3, 9), dtype=np.int64)
    with pytest.raises(ValueError, match='boundary'):
        ins.calculate_log_probability(ok, boundary='reuse')
    for bad in (ok.astype(np.float64), ok[:, :8], ok[0], ok.tolist()):
        with pytest.raises(ValueError):
            ins.calculate_log_probability(bad)
    b = ok.copy()
    b[2, 4] = 2 if make is ising else 3                  # model cell 4 has 2 states (Ising: the inactive spin) / 3 (RMF)
    with pytest.raises(ValueError, match=r'states\[2, 4\]'):
        ins.calculate_log_probability(b)
    b[2, 4] = -1
    with pytest.raises(ValueError, match='outside'):
        ins.calculate_log_probability(b)
    with pytest.raises(ValueError):                      # states=None on a solver without stored states: nothing to score
        ins.calculate_log_probability()
    with pytest.raises(ValueError, match='chunk'):
        ins.calculate_log_probability(ok, chunk=0)
    with pytest.raises(ValueError, match='rhoT'):
        ins.calculate_log_probability(ok, boundary='keep')
    assert not hasattr(ins, 'scored_log2q') and not hasattr(ins, 'rhoT')


def test_calculate_free_energy_validates_before_any_device_work():
    ins = ising()
    with pytest.raises(ValueError, match='boundary'):
        ins.calculate_free_energy(boundary='reuse')
    with pytest.raises(ValueError, match='rhoT and rhoB'):
        ins.calculate_free_energy(boundary='keep')
    assert not hasattr(ins, 'log2Z') and not hasattr(ins, 'rhoT')


# ---------------------------------------------------------------------------------------------- argument errors of the exports
def _lib():
    from tnac4o_amd import _lib
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _expect_neg(L, rc, text):
    assert rc < 0, rc
    buf = ctypes.create_string_buffer(256)
    L.tn_last_error(buf, 256)
    assert text in buf.value.decode(), buf.value.decode()


def test_score_pn_argument_errors():
    L = _lib()
    host = (ctypes.c_double * 64)()
    P = ctypes.cast(host, ctypes.c_void_p)               # a host address standing in for device memory: never dereferenced

    def sp(T1=P, perm=P, starts=P, forced=P, child=P, lq=P, cl=None, mp=P, ng=4, ld=16, pos=3, q=16, nl=1, nu=1, p=1, Dr=1, br=1):
        return L.tn_score_pn(T1, P, P, P, P, P, P, P, P, perm, starts, ng, forced, ld, pos, q, nl, nu, p, Dr, br, child, lq, cl, mp, None)
    for kw in ({'T1': None}, {'perm': None}, {'starts': None}, {'forced': None}, {'child': None}, {'lq': None}, {'mp': None}):
        _expect_neg(L, sp(**kw), 'null operand')
    _expect_neg(L, sp(ng=-1), 'negative group count')
    _expect_neg(L, sp(q=0), 'non-positive dimension')
    _expect_neg(L, sp(pos=16), 'column outside')
    _expect_neg(L, sp(pos=-1), 'column outside')
    _expect_neg(L, sp(q=256, p=64, Dr=512, br=64), 'LDS')
    _expect_neg(L, sp(q=19189, p=2, Dr=2, br=2), 'LDS')                  # one state more than tn_calc_pn's bound admits
    assert sp(q=19188, p=2, Dr=2, br=2, ng=0) == 0
    assert sp(ng=0) == 0                                                 # nothing to do: no launch


def test_gibbs_score_argument_errors():
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

    def gs(cl=cells, M=8, B=4, st=P, E=P, lq=P, clq=None, gm=ctypes.byref(gmin), ws=P, wsb=big):
        return L.tn_gibbs_score(1, 1, ctypes.cast(cl, ctypes.c_void_p) if cl is not None else None, M, B, st, E, lq, clq, gm, ctypes.byref(mg),
                                ws, wsb, None)
    # the workspace is the sampling walk's own
    assert L.tn_gibbs_score_ws_bytes(4, 4, 64, 256, 64, 64, 256) == L.tn_gibbs_sample_ws_bytes(4, 4, 64, 256, 64, 64, 256) > 0
    _expect_neg(L, gs(cl=None), 'bad arguments')
    _expect_neg(L, gs(M=0), 'bad arguments')
    _expect_neg(L, gs(B=0), 'bad arguments')
    _expect_neg(L, gs(ws=None), 'bad arguments')
    _expect_neg(L, gs(M=1 << 31), 'too many samples')
    _expect_neg(L, gs(st=None), 'states')
    for kw in ({'E': None}, {'lq': None}, {'gm': None}):
        _expect_neg(L, gs(**kw), 'null result pointer')
    _expect_neg(L, gs(M=1 << 20, B=1 << 12), 'exceeds int64')
    need = L.tn_gibbs_score_ws_bytes(1, 1, 8, 4, 2, 4, 2)
    rc = gs(wsb=need - 8)
    assert rc == -3
    _expect_neg(L, rc, 'tn_gibbs_score: workspace too small')
    c.q = 40000
    _expect_neg(L, gs(), 'bad cell')
    c.q, c.p = 4, 3
    _expect_neg(L, gs(), 'vertical bond')
    c.p, c.q = 2, 9700                                   # too large for the draw's table + running sum, fine for the score
    _expect_neg(L, L.tn_gibbs_sample(1, 1, ctypes.cast(cells, ctypes.c_void_p), 8, 4, P, 8, P, P, P, ctypes.byref(gmin), ctypes.byref(mg), P, 0,
                                     None), 'LDS')
    assert gs(wsb=0) == -3
    c.q = 19200
    _expect_neg(L, gs(), 'LDS')
