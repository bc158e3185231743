"""GPU tests of tn_svd_trunc (csrc/svd.hip) on its three paths -- svd_trunc_small_kernel (both sides <= 64), the block path with
all rounds in one launch (TN_SVD_SMALL=0) and with separate launches (TN_SVD_SMALL=0, TN_SVD_FUSED=0; both switches are read per
call) -- against the 40-digit reference, the inputs and the settings of tests/svd_trunc_ref.py.  Every call goes through the
C-ABI; U, S, Vt and the workspace are framed by guard bytes (tests/guarded.py) and the outputs pre-filled with NaN bit patterns,
so a write past an output, a write beyond the first `keep` vectors, or a kept element left unwritten shows.

Bounds (the ones the project already holds these kernels to):
- values: 1e-13 S0 (check_svd and test_small_truncated_svd_single_launch in tests/test_gpu_kernels.py, tests/test_gpu_svdvals.py);
- orthonormality: 5e-13 (check_svd); 1e-13 on the one-launch path (test_small_truncated_svd_single_launch);
- discarded weight: 1e-6 relative + 1e-14 absolute (check_svd);
- U S Vt - A: 1e-12 S0 + 1.01 S_keep (test_small_truncated_svd_single_launch), and the same 1e-12 S0 for the two residuals
  U^T A - S Vt and A Vt^T - U S, which with orthonormality make every kept pair a singular pair to that backward error."""
import ctypes as ct

import numpy as np
import pytest

import svd_trunc_ref as tr
import svdvals_ref as sv

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
from guarded import Guarded, same_bits  # noqa: E402
from test_gpu_svdvals import dev_view, run_sync, _svdvals_batched  # noqa: E402

F64 = torch.float64
NAN, INF = float('nan'), float('inf')
FILL = np.uint64(0xFFFFFFFFFFFFFFFF)
CASES = tr.cases()
PATH_ENV = {'small': {}, 'block': {'TN_SVD_SMALL': '0'}, 'block_separate': {'TN_SVD_SMALL': '0', 'TN_SVD_FUSED': '0'}}
TRIPLES = [(name, Dmax, tol, path) for name, A in CASES.items() for Dmax, tol in tr.settings(name, A) for path in tr.paths(A)]


def on_paths(names):
    """(name, path) for every path the case can take (a side >= 65 leaves only the block path)."""
    return [(name, path) for name in names for path in tr.paths(CASES[name])]


def shape_paths(shapes):
    return [(sh, path) for sh in shapes for path in tr.paths(np.empty(sh))]


@pytest.fixture(scope='module')
def L():
    from tnac4o_amd import _lib
    return _lib.lib()


@pytest.fixture
def on_path(monkeypatch):
    def set_path(path):
        for var in ('TN_SVD_SMALL', 'TN_SVD_FUSED'):
            monkeypatch.delenv(var, raising=False)
        for var, val in PATH_ENV[path].items():
            monkeypatch.setenv(var, val)
    return set_path


def _st():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _msg(L):
    buf = ct.create_string_buffer(256)
    L.tn_last_error(buf, 256)
    return buf.value.decode()


def _ids(v):
    return '%g' % v if isinstance(v, float) else str(v)


class Out:
    """One output matrix (rows x cols logical, the first `keep` of its `cap` vectors to be written) in a guarded, NaN-filled array.
    vec_axis: the axis the kept vectors are counted along (U: 1, Vt: 0).  layout 'c': contiguous; 'pad': a longer leading dimension
    (pad more elements per row); 't': stored transposed."""

    def __init__(self, rows, cols, vec_axis, layout, pad):
        self.shape, self.vec_axis = (rows, cols), vec_axis
        if layout == 't':
            self.phys = (cols, rows)
            self.rs, self.cs = 1, rows
        else:
            self.phys = (rows, cols + (pad if layout == 'pad' else 0))
            self.rs, self.cs = self.phys[1], 1
        self.layout = layout
        self.g = Guarded.of(F64, self.phys)

    def read(self, keep):
        """The kept part (host); asserts that it is finite and that every other element still has its fill bits."""
        assert self.g.intact()
        H = self.g.host()
        logical = H.T if self.layout == 't' else H[:, :self.shape[1]]
        mask = np.zeros(self.phys, dtype=bool)
        lm = mask.T if self.layout == 't' else mask[:, :self.shape[1]]
        if self.vec_axis == 1:
            lm[:, :keep] = True
            kept = logical[:, :keep]
        else:
            lm[:keep, :] = True
            kept = logical[:keep, :]
        assert np.all(np.isfinite(H[mask])), 'a kept element is not finite (left unwritten?)'
        assert np.all(H.view(np.uint64)[~mask] == FILL), 'an element beyond the kept vectors or in the padding was written'
        return np.ascontiguousarray(kept)


def call(L, Cm, Dmax, tol, ul='c', vl='c'):
    """tn_svd_trunc on the device matrix Cm: dict of rc, the host results and (for rc == 0) the kept U, S, Vt."""
    k, n = Cm.shape
    cap = min(k, n, Dmax)
    U = Out(k, cap, 1, ul, 3)
    V = Out(cap, n, 0, vl, 5)
    S = Guarded.of(F64, (cap,))
    wsb = int(L.tn_svd_ws_bytes(k, n, 1))
    ws = Guarded(wsb)
    keep, disc, sweeps, info = ct.c_int64(-1), ct.c_double(-7.0), ct.c_int(-1), ct.c_int(-1)
    rc = L.tn_svd_trunc(Cm.data_ptr(), Cm.stride(0), Cm.stride(1), k, n, Dmax, tol, U.g.ptr, U.rs, U.cs, S.ptr, V.g.ptr, V.rs, V.cs,
                        ct.byref(keep), ct.byref(disc), ct.byref(sweeps), ct.byref(info), ws.ptr, wsb, _st())
    torch.cuda.synchronize()
    assert ws.intact() and S.intact()
    r = {'rc': rc, 'keep': keep.value, 'disc': disc.value, 'sweeps': sweeps.value, 'info': info.value, 'cap': cap}
    kk = keep.value if rc == 0 else 0
    assert 0 <= kk <= cap, (kk, cap)
    r['U'], r['Vt'] = U.read(kk), V.read(kk)
    Sh = S.host()
    assert np.all(np.isfinite(Sh[:kk])) and np.all(Sh.view(np.uint64)[kk:] == FILL)
    r['S'] = Sh[:kk].copy()
    return r


def same_result(a, b):
    return (a['rc'] == b['rc'] and a['keep'] == b['keep'] and a['sweeps'] == b['sweeps'] and a['info'] == b['info']
            and same_bits(np.float64(a['disc']), np.float64(b['disc'])) and same_bits(a['U'], b['U']) and same_bits(a['S'], b['S'])
            and same_bits(a['Vt'], b['Vt']))


def gauge_holds(U, Vt):
    """The reference's sign gauge: no column of U and row of Vt both have a most negative entry outweighing the most positive."""
    if U.shape[1] == 0:
        return True
    return not np.any((np.abs(U.min(0)) > U.max(0)) & (np.abs(Vt.min(1)) > Vt.max(1)))


def check_factors(tag, A, sigma, r, name, Dmax, tol, path, scale_exp=0):
    """What a call owes on a finite input.  scale_exp = e: the call ran on 2^e A; the values are held to 2^e sigma and the residuals
    are evaluated on A and 2^-e S, so that the check itself stays in range."""
    s0 = sigma[0]
    keep = r['keep']
    print(tag, 'keep', keep, 'disc', r['disc'], 'sweeps', r['sweeps'])
    assert r['rc'] == 0 and r['info'] == 0, tag
    assert (0 if s0 == 0.0 else 1) <= r['sweeps'] <= 40, (tag, r['sweeps'])
    lo, hi = tr.keep_bounds(name, sigma, Dmax, tol)
    assert lo <= keep <= hi, (tag, keep, lo, hi)
    want = tr.discarded_at(sigma, keep)
    print(tag, 'discarded', r['disc'], 'reference', want)
    assert abs(r['disc'] - want) <= 1e-6 * want + 1e-14, (tag, r['disc'], want)
    U, Vt = r['U'], r['Vt']
    S = np.ldexp(r['S'], -scale_exp)
    assert np.all(np.ldexp(S, scale_exp) == r['S']), tag         # (the rescaling of the check is exact)
    if keep:
        print(tag, 'value error / s0', np.abs(S - sigma[:keep]).max() / s0)
        assert np.abs(S - sigma[:keep]).max() <= 1e-13 * s0, tag
    assert np.all(np.diff(S) <= 0) and np.all(S > 0), tag
    orth = 1e-13 if path == 'small' else 5e-13
    eu = np.abs(U.T @ U - np.eye(keep)).max() if keep else 0.0
    ev = np.abs(Vt @ Vt.T - np.eye(keep)).max() if keep else 0.0
    res_l = np.abs(U.T @ A - S[:, None] * Vt).max() if keep else 0.0
    res_r = np.abs(A @ Vt.T - U * S[None, :]).max() if keep else 0.0
    rec = np.abs((U * S[None, :]) @ Vt - A).max()
    tail = sigma[keep] if keep < sigma.size else 0.0
    print(tag, 'orth', eu, ev, 'residuals / s0', res_l / max(s0, 1e-300), res_r / max(s0, 1e-300), 'recon', rec, 'tail', tail)
    assert eu <= orth and ev <= orth, (tag, eu, ev)
    assert res_l <= 1e-12 * s0 and res_r <= 1e-12 * s0, (tag, res_l, res_r, s0)
    assert rec <= 1e-12 * s0 + 1.01 * tail, (tag, rec, tail)
    assert gauge_holds(U, Vt), tag


# ------------------------------------------------------------------------------------------------------------------ every path
@pytest.mark.parametrize('name,Dmax,tol,path', TRIPLES, ids=['-'.join(_ids(v) for v in t) for t in TRIPLES])
def test_factors_against_reference(L, on_path, name, Dmax, tol, path):
    on_path(path)
    A = CASES[name]
    sigma = tr.ref_svdvals(A)
    Cm = dev_view(A)
    r = call(L, Cm, Dmax, tol)
    tag = (name, Dmax, tol, path)
    assert r['rc'] == 0, (tag, _msg(L))
    check_factors(tag, np.asarray(A), sigma, r, name, Dmax, tol, path)
    if tol >= 1.0:
        assert r['keep'] == 0
    if name in tr.ZERO:
        assert r['keep'] == 0 and same_bits(np.float64(r['disc']), np.float64(0.0)), tag
    if name in tr.TINY_ROW:
        assert r['keep'] >= 1 and np.all(r['U'][tr.TINY_ROW[name], :] == 0.0), tag          # the deflated input row takes no part
    assert same_result(call(L, Cm, Dmax, tol), r), tag           # a second call: the same bits and host results


# ------------------------------------------------------------------------------------------------------------------ strides
@pytest.mark.parametrize('name,path', on_paths(tr.STRIDE_CASES))
def test_output_strides(L, on_path, name, path):
    """Padded leading dimensions (what the chain driver passes) and transposed outputs: the same bits as the contiguous call, and the
    padding keeps its fill (checked by Out.read)."""
    A = CASES[name]
    on_path(path)
    Cm = dev_view(A)
    for Dmax in (min(A.shape), 20):
        base = call(L, Cm, Dmax, 0.0)
        assert base['rc'] == 0 and base['keep'] == Dmax, (name, path, _msg(L))
        for ul, vl in (('pad', 'c'), ('t', 'c'), ('c', 'pad'), ('c', 't'), ('t', 'pad')):
            assert same_result(call(L, Cm, Dmax, 0.0, ul, vl), base), (name, path, Dmax, ul, vl)


@pytest.mark.parametrize('name,path', on_paths(tr.STRIDE_CASES + ('gauss_17x17', 'gauss_3x5', 'gauss_3x65', 'gauss_65x3')))
def test_input_orientation(L, on_path, name, path):
    """C contiguous against the same matrix as the transposed view of C^T stored contiguously: the same bits."""
    A = CASES[name]
    on_path(path)
    Cm = dev_view(A)
    Ct = Cm.t().contiguous().t()
    assert Ct.shape == Cm.shape and Ct.stride(0) == 1 and torch.equal(Ct, Cm)
    Dmax = min(A.shape)
    base = call(L, Cm, Dmax, 0.0)
    assert base['rc'] == 0, _msg(L)
    assert same_result(call(L, Ct, Dmax, 0.0), base), (name, path)


# ------------------------------------------------------------------------------------------------------------------ batched
def _batched(L, items, Dmax, tol):
    """tn_svd_trunc_batched on equally shaped host matrices, every batch stride padded; NaN between the items of C."""
    b = len(items)
    k, n = items[0].shape
    cap = min(k, n, Dmax)
    bsC, bsU, bsS, bsV = k * n + 7, k * cap + 5, cap + 3, cap * n + 9
    Ch = np.full(b * bsC, NAN)
    for i, A in enumerate(items):
        Ch[i * bsC:i * bsC + k * n] = A.ravel()
    Cd = torch.as_tensor(Ch, dtype=F64).cuda()
    U, S, V = Guarded.of(F64, (b, bsU)), Guarded.of(F64, (b, bsS)), Guarded.of(F64, (b, bsV))
    wsb = -(-int(L.tn_svd_ws_bytes(k, n, 1)) // 256) * 256
    ws = Guarded(wsb)
    keep = (ct.c_int64 * b)(*([-1] * b))
    disc = (ct.c_double * b)(*([-7.0] * b))
    sweeps = (ct.c_int * b)(*([-1] * b))
    info = (ct.c_int * b)(*([-1] * b))
    rc = L.tn_svd_trunc_batched(Cd.data_ptr(), n, 1, k, n, Dmax, tol, U.ptr, cap, 1, S.ptr, V.ptr, n, 1, keep, disc, sweeps, info, b,
                                bsC, bsU, bsS, bsV, ws.ptr, wsb, _st())
    torch.cuda.synchronize()
    assert ws.intact() and U.intact() and S.intact() and V.intact()
    Uh, Sh, Vh = U.host(), S.host(), V.host()
    out = []
    for i in range(b):
        kk = keep[i] if keep[i] >= 0 else 0
        Ui, Vi = Uh[i, :k * cap].reshape(k, cap), Vh[i, :cap * n].reshape(cap, n)
        untouched = (np.all(Uh[i].view(np.uint64) == FILL) and np.all(Sh[i].view(np.uint64) == FILL)
                     and np.all(Vh[i].view(np.uint64) == FILL))
        rest = (np.all(Ui[:, kk:].view(np.uint64) == FILL) and np.all(Uh[i, k * cap:].view(np.uint64) == FILL)
                and np.all(Sh[i, kk:].view(np.uint64) == FILL) and np.all(Vi[kk:].view(np.uint64) == FILL)
                and np.all(Vh[i, cap * n:].view(np.uint64) == FILL))
        out.append({'rc': 0, 'keep': keep[i], 'disc': disc[i], 'sweeps': sweeps[i], 'info': info[i], 'U': np.ascontiguousarray(Ui[:, :kk]),
                    'S': Sh[i, :kk].copy(), 'Vt': np.ascontiguousarray(Vi[:kk]), 'untouched': untouched, 'rest_untouched': rest})
    return rc, out


@pytest.mark.parametrize('shape,path', shape_paths(tr.BATCH_SHAPES))
def test_batched_equals_single_calls(L, on_path, shape, path):
    """Each item of tn_svd_trunc_batched equals its single call bit for bit; a NaN or an Inf in item 1 ends the call with -2 after
    item 0 was delivered, and items 1 and 2 of U, S, Vt and keep_host[2] are left as they were."""
    items = tr.batch_items(shape)
    on_path(path)
    Dmax, tol = 12, 0.0
    singles = [call(L, torch.as_tensor(A, dtype=F64).cuda(), Dmax, tol) for A in items]
    rc, out = _batched(L, items, Dmax, tol)
    assert rc == 0, _msg(L)
    for i in range(len(items)):
        assert singles[i]['rc'] == 0 and singles[i]['keep'] == Dmax
        assert out[i]['rest_untouched'], (shape, path, i)
        assert same_result(out[i], singles[i]), (shape, path, i)
    for bad in (NAN, INF):
        poisoned = [A.copy() for A in items]
        poisoned[1][shape[0] // 2, (2 * shape[1]) // 3] = bad
        rc, out = _batched(L, poisoned, Dmax, tol)
        assert rc == -2 and 'svd: non-finite input' in _msg(L), (rc, _msg(L))
        assert out[0]['rest_untouched'] and same_result(out[0], singles[0]), (shape, path, bad)
        assert out[1]['untouched'] and out[2]['untouched'], (shape, path, bad)
        assert out[2]['keep'] == -1


# ------------------------------------------------------------------------------------------------------------------ non-finite input
@pytest.mark.parametrize('bad', (NAN, INF), ids=('nan', 'inf'))
@pytest.mark.parametrize('where', ('interior', 'corner'))
@pytest.mark.parametrize('shape,path', shape_paths(tr.NONFINITE_SHAPES))
def test_nonfinite_input_is_reported(L, on_path, shape, where, bad, path):
    """-2 'svd: non-finite input' and no output element touched, wherever the entry sits."""
    A = tr.nonfinite_base(shape).copy()
    on_path(path)
    k, n = shape
    A[{'interior': (k // 2, (2 * n) // 3), 'corner': (k - 1, n - 1)}[where]] = bad
    r = call(L, torch.as_tensor(A, dtype=F64).cuda(), min(shape), 0.0)      # (call asserts that nothing was written when rc != 0)
    assert r['rc'] == -2 and 'svd: non-finite input' in _msg(L), (r['rc'], _msg(L))


# ------------------------------------------------------------------------------------------------------------------ zero
@pytest.mark.parametrize('name,path', on_paths(tr.ZERO))
def test_zero_input(L, on_path, name, path):
    """An all-zero matrix: rc 0, keep = 0, a discarded weight of exactly 0.0 (not the NaN of 0 / 0), nothing written."""
    A = CASES[name]
    on_path(path)
    for Dmax, tol in ((min(A.shape), 0.0), (10 ** 6, 1e-16), (3, 1e-3), (10 ** 6, 1.0)):
        r = call(L, dev_view(A), Dmax, tol)                      # (call asserts that everything beyond keep = 0 kept its fill)
        assert r['rc'] == 0 and r['keep'] == 0 and r['info'] == 0 and 0 <= r['sweeps'] <= 40, (name, path, r, _msg(L))
        assert same_bits(np.float64(r['disc']), np.float64(0.0)), (name, path, r['disc'])


@pytest.mark.parametrize('name', tr.ZERO)
def test_zero_input_values_only(L, name):
    """The values-only twin on the same inputs: zeros, no NaN."""
    A = CASES[name]
    rc, S, sweeps, info = run_sync(L, dev_view(A))
    assert rc == 0 and same_bits(S, np.zeros(min(A.shape))) and info == 0, (name, S, _msg(L))


# ------------------------------------------------------------------------------------------------------------------ range
RANGE_SETTINGS = (('full', None, 0.0), ('cut', 16, 0.0), ('tol', 10 ** 6, 0.4))


@pytest.mark.parametrize('path', list(PATH_ENV))
@pytest.mark.parametrize('e', sv.RANGE_EXPONENTS)
def test_full_double_range(L, on_path, e, path):
    """C = 2^e base over the whole double range (24 x 40 on the one-launch path, 65 x 66 on the block path): rank, discarded weight,
    orthonormality, sign gauge and residuals as for the base, values within 1e-13 2^e S0 of 2^e sigma.  Every path scales by powers of
    two only (the one-launch kernel always; the block path when the largest squared norm leaves 2^-320 .. 2^500, and inside that window
    its arithmetic consists of products, sums, rsq / rcp seeds and Newton steps, all of which commute with a power of two while nothing
    under- or overflows), so U and Vt have the bits of the base's and S = 2^e S_base exactly: 2^e sigma_min is a normal number for
    every exponent of the list."""
    on_path(path)
    A = tr.range_base(path)
    sigma = tr.ref_svdvals(A)
    assert np.ldexp(sigma[-1], e) > 2.3e-308 and np.ldexp(sigma[0], e) < 1e308
    Cb, Ce = dev_view(A), dev_view(np.ldexp(A, e))
    for label, Dmax, tol in RANGE_SETTINGS:
        Dmax = min(A.shape) if Dmax is None else Dmax
        thr = sigma[0] * max(tr.EPS, tol)
        assert not np.any(np.abs(sigma - thr) <= tr.MARGIN * thr)            # the margin condition, as for the cases
        base = call(L, Cb, Dmax, tol)
        r = call(L, Ce, Dmax, tol)
        tag = ('range', e, path, label)
        assert r['rc'] == 0, (tag, _msg(L))
        check_factors(tag + ('base',), A, sigma, base, 'range', Dmax, tol, path)
        check_factors(tag, A, sigma, r, 'range', Dmax, tol, path, scale_exp=e)
        assert 1 <= r['keep'] == base['keep'] and (label == 'full' or r['keep'] < min(A.shape)), tag
        assert same_bits(r['U'], base['U']) and same_bits(r['Vt'], base['Vt']), tag
        assert same_bits(r['S'], np.ldexp(base['S'], e)), tag
        assert r['sweeps'] == base['sweeps'] and same_bits(np.float64(r['disc']), np.float64(base['disc'])), tag


@pytest.mark.parametrize('e', sv.RANGE_EXPONENTS)
def test_full_double_range_values_only(L, e):
    """tn_svdvals and tn_svdvals_batched above 64 (the block path) on the same 65 x 66 inputs: the same value bound."""
    A = tr.range_base('block')
    k, n = A.shape
    sigma = tr.ref_svdvals(A)
    rc0, S0, sweeps0, info0 = run_sync(L, dev_view(A))
    rc, S, sweeps, info = run_sync(L, dev_view(np.ldexp(A, e)))
    assert rc0 == 0 and rc == 0, _msg(L)
    assert info == 0 and 1 <= sweeps <= 40
    print('values only', e, np.abs(np.ldexp(S, -e) - sigma).max() / sigma[0])
    assert np.abs(S - np.ldexp(sigma, e)).max() <= 1e-13 * np.ldexp(sigma[0], e), (e, S[:4])
    assert np.all(np.diff(S) <= 0) and np.all(S > 0)
    assert same_bits(S, np.ldexp(S0, e)) and sweeps == sweeps0, e
    bs = k * n + 37
    buf = np.full(2 * bs, NAN)
    buf[:k * n] = np.ldexp(A, e).ravel()
    buf[bs:bs + k * n] = A.ravel()
    rc, Sb, sw, inf_ = _svdvals_batched(L, torch.as_tensor(buf, dtype=F64).cuda(), k, n, 2, bs)
    assert rc == 0, _msg(L)
    assert same_bits(Sb[0], S) and same_bits(Sb[1], S0) and sw == [sweeps, sweeps0] and inf_ == [0, 0], e
