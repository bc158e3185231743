"""GPU tests of the values-only SVD of small centre matrices -- one device routine (svd_vals_small_body, csrc/svd.hip) behind
tn_svdvals (sides <= 64), tn_svdvals_async and tn_svdvals_small_batched -- and of tn_svdvals_batched, against the 40-digit
reference and the inputs of tests/svdvals_ref.py.  Every export is called through the C-ABI; device outputs are framed by guard
bytes (tests/guarded.py) and pre-filled with NaN, so a write past an output or an element left unwritten shows.  Bound on the
values: 1e-13 S0, the one the oracle and the truncating twin (svd_trunc_small_kernel) are held to."""
import ctypes as ct
import math

import numpy as np
import pytest

import svdvals_ref as sv

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
from guarded import Guarded, same_bits  # noqa: E402

F64 = torch.float64
TOL = 1e-13
SENT = 0x5A
CASES = sv.cases()
EXACT = sv.exact_cases()
INPUTS = dict(CASES, **{k: v[0] for k, v in EXACT.items()})
NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def L():
    from tnac4o_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def ops():
    from tnac4o_amd import ops as o
    return o


def _st():
    return ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _msg(L):
    buf = ct.create_string_buffer(256)
    L.tn_last_error(buf, 256)
    return buf.value.decode()


def dev_view(A):
    """A on the device with the strides it has on the host (the owning array is uploaded as it lies in memory)."""
    if A.flags['C_CONTIGUOUS']:
        return torch.as_tensor(A, dtype=F64).cuda()
    root, off, strides = sv.root_and_view(A)
    assert root.flags['C_CONTIGUOUS'] or root.flags['F_CONTIGUOUS']
    flat = torch.as_tensor(np.ascontiguousarray(root.ravel(order='K')), dtype=F64).cuda()
    return torch.as_strided(flat, A.shape, strides, off)


def _desc(mats):
    d = np.empty((len(mats), 5), dtype=np.int64)
    for i, Cm in enumerate(mats):
        k, n = Cm.shape
        d[i] = (Cm.data_ptr(), Cm.stride(0), Cm.stride(1), k, n) if k <= n else (Cm.data_ptr(), Cm.stride(1), Cm.stride(0), n, k)
    return d


def run_async(L, Cm):
    """The 66 doubles of tn_svdvals_async; exactly those are written."""
    k, n = Cm.shape
    out = Guarded.of(F64, (66,))
    assert L.tn_svdvals_async(Cm.data_ptr(), Cm.stride(0), Cm.stride(1), k, n, out.ptr, _st()) == 0, _msg(L)
    torch.cuda.synchronize()
    assert out.intact()
    h = out.host()
    assert not same_bits(h[64:], np.frombuffer(b'\xff' * 16, dtype=np.float64))         # sweeps and flag were written
    return h


def run_batched(L, mats):
    """The (batch, 66) table of tn_svdvals_small_batched; exactly 66 batch doubles are written."""
    b = len(mats)
    desc = _desc(mats)
    ddesc = torch.from_numpy(desc).cuda()
    out = Guarded.of(F64, (b, 66))
    assert L.tn_svdvals_small_batched(ddesc.data_ptr(), b, desc.ctypes.data_as(ct.c_void_p), out.ptr, _st()) == 0, _msg(L)
    torch.cuda.synchronize()
    assert out.intact()
    return out.host()


def run_sync(L, Cm):
    """tn_svdvals: (rc, min(k, n) values, sweeps, info); the host array is framed by sentinels."""
    k, n = Cm.shape
    nv = min(k, n)
    wsb = L.tn_svd_ws_bytes(k, n, 0)
    ws = Guarded(wsb)
    S = np.full(nv + 8, -7.0)
    sweeps, info = ct.c_int(-1), ct.c_int(-1)
    rc = L.tn_svdvals(Cm.data_ptr(), Cm.stride(0), Cm.stride(1), k, n, S[4:].ctypes.data_as(ct.POINTER(ct.c_double)), ct.byref(sweeps),
                      ct.byref(info), ws.ptr, wsb, _st())
    torch.cuda.synchronize()
    assert ws.intact()
    assert np.all(S[:4] == -7.0) and np.all(S[4 + nv:] == -7.0)
    return rc, S[4:4 + nv].copy(), sweeps.value, info.value


def as66(S, sweeps, info):
    out = np.zeros(66)
    out[:S.size] = S
    out[64], out[65] = float(sweeps), float(info == 0)
    return out


_single = {}


def single(L, name):
    """The 66 doubles of tn_svdvals_async on input `name` (taken once per module)."""
    if name not in _single:
        _single[name] = run_async(L, dev_view(INPUTS[name]))
    return _single[name]


def check_values(name, out, A, ref):
    """What every entry point owes on a finite input: values within TOL S0 of the reference, descending, >= 0, zero padded, a sweep
    count in 1..40 and the convergence flag."""
    nv = min(A.shape)
    S = out[:nv]
    assert np.all(np.isfinite(out)), name
    assert np.abs(S - ref).max() <= TOL * ref[0], (name, np.abs(S - ref).max(), ref[0])
    assert np.all(np.diff(S) <= 0) and np.all(S >= 0), name
    assert same_bits(out[nv:64], np.zeros(64 - nv)), name
    assert out[64] == int(out[64]) and 1 <= out[64] <= 40, (name, out[64])
    assert out[65] == 1.0, name


# ------------------------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize('name', list(INPUTS))
def test_accuracy_three_entry_points(L, name):
    A = INPUTS[name]
    ref = sv.ref_svdvals(A)
    Cm = dev_view(A)
    outs = {'async': single(L, name), 'batched': run_batched(L, [Cm])[0]}
    rc, S, sweeps, info = run_sync(L, Cm)
    assert rc == 0, _msg(L)
    outs['sync'] = as66(S, sweeps, info)
    for entry, out in outs.items():
        check_values((name, entry), out, A, ref)
        if name == 'zero':
            assert same_bits(out[:64], np.zeros(64)), entry
        if name == 'tiny_row':
            assert out[9] == 0.0, entry                          # the deflated row is reported as 0
        if name in EXACT:
            nv = min(A.shape)
            assert same_bits(out[:nv], EXACT[name][1]) and out[64] == 1.0, (name, entry, out[64])


@pytest.mark.parametrize('name', list(INPUTS))
def test_one_body_same_bits(L, name):
    """async, batched with batch 1 and tn_svdvals give the same 66 doubles, and so do a contiguous copy of C and the transposed view
    of C^T made contiguous: the host resolves the orientation to the same vectors."""
    A = INPUTS[name]
    Cm = dev_view(A)
    base = single(L, name)
    for form, M in (('as given', Cm), ('contiguous', Cm.contiguous()), ('transposed view', Cm.t().contiguous().t())):
        assert M.shape == Cm.shape
        if form == 'transposed view' and min(A.shape) > 1:
            assert M.stride(0) == 1
        assert same_bits(run_async(L, M), base), (name, form)
        assert same_bits(run_batched(L, [M])[0], base), (name, form)
        rc, S, sweeps, info = run_sync(L, M)
        assert rc == 0, _msg(L)
        assert same_bits(as66(S, sweeps, info), base), (name, form)


# ------------------------------------------------------------------------------------------------------------------ batching
def _batch_items(batch):
    """(key, device matrix) per item: the inputs in turn; from batch 2 on two neighbouring items (from batch 7 on: also the last) are
    different views of ONE storage."""
    names = list(INPUTS)
    step = next(s for s in (5, 7, 9, 11, 13) if math.gcd(s, len(names)) == 1)
    shared = torch.as_tensor(np.random.default_rng(77).standard_normal((50, 90)), dtype=F64).cuda()
    views = {'shared_a': shared[:40, 10:70:2], 'shared_b': shared[10:50, 20:84], 'shared_c': shared.t()[26:90, 3:50:3]}
    items = []
    pos = {2: (0, 1)}.get(batch, (1, 2) if batch > 2 else ())
    for i in range(batch):
        if i in pos:
            key = 'shared_a' if i == pos[0] else 'shared_b'
        elif batch >= 7 and i == batch - 1:
            key = 'shared_c'
        else:
            key = names[(i * step) % len(names)]                # a step coprime to the number of inputs: neighbours differ in shape and kind
        items.append((key, views[key] if key in views else dev_view(INPUTS[key])))
    return items


@pytest.mark.parametrize('batch', (1, 2, 7, 300))
def test_batched_rows_equal_single_calls(L, batch):
    """Row i of the batched table equals the single asynchronous call on item i bit for bit, whatever its neighbours (300 items:
    more workgroups than the device has compute units)."""
    items = _batch_items(batch)
    table = run_batched(L, [m for _, m in items])
    assert table.shape == (batch, 66)
    singles = {}
    for i, (key, M) in enumerate(items):
        if key not in singles:
            singles[key] = single(L, key) if key in INPUTS else run_async(L, M)
        assert same_bits(table[i], singles[key]), (batch, i, key)
    if batch >= 7:
        assert len({k for k, _ in items}) >= min(batch, 7)


# ------------------------------------------------------------------------------------------------------------------ tn_svdvals_batched
def _strided_batch(k, n, batch, rng, gap=37):
    """batch Gaussian k x n items at a batch stride of k n + gap, NaN in the gaps."""
    bs = k * n + gap
    buf = np.full(batch * bs, NAN)
    for i in range(batch):
        buf[i * bs:i * bs + k * n] = rng.standard_normal(k * n)
    return buf, bs


def _svdvals_batched(L, Cd, k, n, batch, bs, nullable=False):
    nv = min(k, n)
    wsb = L.tn_svd_ws_bytes(k, n, 0)
    ws = Guarded(wsb)
    S = np.full(batch * nv + 8, -7.0)
    sw = (ct.c_int * max(batch, 1))(*([-1] * max(batch, 1)))
    info = (ct.c_int * max(batch, 1))(*([-1] * max(batch, 1)))
    rc = L.tn_svdvals_batched(Cd.data_ptr(), n, 1, k, n, S[4:].ctypes.data_as(ct.POINTER(ct.c_double)), None if nullable else sw,
                              None if nullable else info, batch, bs, ws.ptr, wsb, _st())
    torch.cuda.synchronize()
    assert ws.intact()
    assert np.all(S[:4] == -7.0) and np.all(S[4 + batch * nv:] == -7.0)
    return rc, S[4:4 + batch * nv].reshape(batch, nv).copy(), list(sw), list(info)


@pytest.mark.parametrize('shape', [(16, 16), (64, 64), (65, 64), (70, 130)])
def test_svdvals_batched_equals_single_calls(L, shape):
    k, n = shape
    batch = 3
    buf, bs = _strided_batch(k, n, batch, np.random.default_rng(k * 1000 + n))
    Cd = torch.as_tensor(buf, dtype=F64).cuda()
    rc, S, sw, info = _svdvals_batched(L, Cd, k, n, batch, bs)
    assert rc == 0, _msg(L)
    for i in range(batch):
        item = Cd[i * bs:i * bs + k * n].view(k, n)
        rc1, S1, sw1, info1 = run_sync(L, item)
        assert rc1 == 0, _msg(L)
        assert same_bits(S[i], S1) and sw[i] == sw1 and info[i] == info1 == 0, (shape, i)
        full = np.linalg.svd(item.cpu().numpy(), compute_uv=False)
        assert np.abs(S[i] - full).max() <= TOL * full[0], (shape, i)
    rc, S2, _, _ = _svdvals_batched(L, Cd, k, n, batch, bs, nullable=True)          # null sweeps_host / info_host
    assert rc == 0, _msg(L)
    assert same_bits(S2, S)
    rc, S0, sw0, info0 = _svdvals_batched(L, Cd, k, n, 0, bs)                        # batch = 0: nothing is touched
    assert rc == 0 and S0.size == 0 and sw0 == [-1] and info0 == [-1]


# ------------------------------------------------------------------------------------------------------------------ path boundary
@pytest.mark.parametrize('name', list(sv.boundary_cases()))
def test_path_boundary(L, name):
    """64 rows: the single launch (longer side <= 64); 65 rows: the block path.  Both within the same bound of the reference."""
    A = sv.boundary_cases()[name]
    assert max(A.shape) == int(name[-2:])
    ref = sv.ref_svdvals(A)
    rc, S, sweeps, info = run_sync(L, dev_view(A))
    assert rc == 0, _msg(L)
    assert info == 0 and sweeps >= 1
    assert np.abs(S - ref).max() <= TOL * ref[0], (name, np.abs(S - ref).max(), ref[0])
    assert np.all(np.diff(S) <= 0) and np.all(S >= 0)


# ------------------------------------------------------------------------------------------------------------------ range
@pytest.mark.parametrize('e', sv.RANGE_EXPONENTS)
def test_full_double_range(L, e):
    """S(2^e A) = 2^e S(A) bit for bit (sweeps and flag included) through all three entry points: the kernel scales its input by a
    power of two, so it sees the same mantissas.  And within the bound of the reference of A."""
    A = sv.range_base()
    nv = min(A.shape)
    ref = sv.ref_svdvals(A)
    base = run_async(L, dev_view(A))
    check_values('range base', base, A, ref)
    Cm = dev_view(np.ldexp(A, e))
    want = base.copy()
    want[:64] = np.ldexp(base[:64], e)
    assert np.all(want[:nv] > 0) and np.all(np.isfinite(want))
    outs = {'async': run_async(L, Cm), 'batched': run_batched(L, [Cm])[0]}
    rc, S, sweeps, info = run_sync(L, Cm)
    assert rc == 0, _msg(L)
    outs['sync'] = as66(S, sweeps, info)
    for entry, out in outs.items():
        assert np.abs(out[:nv] - np.ldexp(ref, e)).max() <= TOL * np.ldexp(ref[0], e), (e, entry, out[:4], want[:4], out[64:])
        assert same_bits(out, want), (e, entry)


# ------------------------------------------------------------------------------------------------------------------ non-finite input
def _poisoned(shape, bad):
    A = sv.nonfinite_base(shape).copy()
    A[shape[0] // 2, (2 * shape[1]) // 3] = bad
    return A


@pytest.mark.parametrize('bad', (NAN, INF), ids=('nan', 'inf'))
@pytest.mark.parametrize('shape', sv.NONFINITE_SHAPES)
def test_nonfinite_input_is_reported(L, ops, shape, bad):
    """tn_svdvals: -2 'svd: non-finite input', ops.svdvals raises; the asynchronous forms: flag 0 and a non-finite value among the first
    min(k, n), which sends their callers (mps._DeferredSchmidt.finish, the chain driver) to the synchronous path."""
    from tnac4o_amd._lib import TnError
    nv = min(shape)
    Cm = dev_view(_poisoned(shape, bad))
    rc, S, sweeps, info = run_sync(L, Cm)
    assert rc == -2 and 'svd: non-finite input' in _msg(L), (rc, _msg(L), S[:4])
    with pytest.raises(TnError, match='svd: non-finite input'):
        ops.svdvals(Cm)
    for entry, out in (('async', run_async(L, Cm)), ('batched', run_batched(L, [Cm])[0])):
        assert out[65] == 0.0, (entry, out[64:], out[:4])
        assert not np.all(np.isfinite(out[:nv])), (entry, out[:nv])


def test_nonfinite_item_leaves_neighbours_alone(L):
    good = ['gauss_7x8', 'gauss_64x64', 'view', 'col_graded']
    mats, keys = [], []
    for i, g in enumerate(good):
        mats.append(dev_view(INPUTS[g]))
        keys.append(g)
        mats.append(dev_view(_poisoned(sv.NONFINITE_SHAPES[i % 2], (NAN, INF)[(i // 2) % 2])))
        keys.append(None)
    table = run_batched(L, mats)
    for i, key in enumerate(keys):
        if key is None:
            nv = min(mats[i].shape)
            assert table[i, 65] == 0.0 and not np.all(np.isfinite(table[i, :nv])), i
        else:
            assert same_bits(table[i], single(L, key)), (i, key)


@pytest.mark.parametrize('bad', (NAN, INF), ids=('nan', 'inf'))
@pytest.mark.parametrize('shape', sv.NONFINITE_SHAPES)
def test_svdvals_batched_stops_at_nonfinite_item(L, shape, bad):
    """-2 at the first non-finite item: the items before it are delivered, the ones after it are not touched."""
    k, n = shape
    nv = min(k, n)
    buf, bs = _strided_batch(k, n, 3, np.random.default_rng(5 + k))
    buf[bs + (k * n) // 2] = bad
    Cd = torch.as_tensor(buf, dtype=F64).cuda()
    rc, S, sw, info = _svdvals_batched(L, Cd, k, n, 3, bs)
    assert rc == -2 and 'svd: non-finite input' in _msg(L), (rc, _msg(L))
    rc1, S1, sw1, info1 = run_sync(L, Cd[:k * n].view(k, n))
    assert rc1 == 0 and same_bits(S[0], S1) and sw[0] == sw1 and info[0] == info1
    assert np.all(S[2] == -7.0) and sw[2] == -1 and info[2] == -1
