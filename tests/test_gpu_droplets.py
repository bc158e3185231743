"""tn_droplets and tnac4o.calculate_droplets on the GPU against the reference of tests/droplets_ref.py.  Integer couplings: every output
bit for bit.  Real couplings: the integer outputs exactly, every energy within (t + 1) 2^-52 sum |terms| of the correctly rounded sum of
its t terms (the reference computes the bound).  The kernel on the shared cases (word edges, the last one-wave row and the first
workgroup row; a path that needs nbits - 1 growth steps, a gap, a star, cliques, isolated spins, one-way arcs, neighbours and arc ranges
out of range, rows with far more droplets than slots; x == ref and its complement; poisoned padding and bits beyond nbits), K = 0,
field and labels null, slicing, and the public call on the small Ising solvers."""
import ctypes as ct

import numpy as np
import pytest

import droplets_ref as dr
import exchange_ref as xr
from guarded import Guarded, same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_gpu_sampling import droplet, dv, small      # noqa: E402  (helpers only, no test is imported)

CASE_IDS = ['%s-%d' % c for c in dr.CASES]
CHIMERA = ('chimera', 128)
INT_KEYS = ('count', 'diff', 'largest', 'root', 'size', 'size_hist', 'labels')


# ---------------------------------------------------------------------------------------------- helpers
def _last_error():
    from tnac4o_amd import _lib
    buf = ct.create_string_buffer(512)
    _lib.lib().tn_last_error(buf, 512)
    return buf.value.decode()


def _framed(dtype, array, seed):
    """A numpy array on the device between guards."""
    array = np.ascontiguousarray(array)
    g = Guarded.of(dtype, array.shape, 0x55, seed=seed)
    if array.size:
        g.tensor().copy_(dv(array))
    return g


def droplets_device(rows, ref, nbits, rowptr, cols, vals, field, K, labels=True, hist=None, pad=0, **unused):
    """One call of tn_droplets with every buffer between guards: the dict of droplets_ref.run (labels None without them).  The outputs
    start as 0x55 bytes: an entry the call left alone shows.  hist: the counts the call adds to (None: zeros).  pad: entries of a row of
    labels behind nbits (ldl = nbits + pad); they must keep their 0x55."""
    from tnac4o_amd import _lib, ops
    L = _lib.lib()
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    M = rows.shape[0]
    g_rows = _framed(torch.int64, rows.view(np.int64), 1)
    g_ref = _framed(torch.int64, np.ascontiguousarray(ref, dtype=np.uint64).view(np.int64), 2)
    g_ptr, g_cols = _framed(torch.int32, np.asarray(rowptr, dtype=np.int32), 3), _framed(torch.int32, np.asarray(cols, dtype=np.int32), 4)
    g_vals = _framed(torch.float64, np.asarray(vals, dtype=np.float64), 5)
    g_field = _framed(torch.float64, np.asarray(field, dtype=np.float64), 6) if field is not None else None
    out = {k: Guarded.of(torch.int32, (M,), 0x55, seed=10 + i) for i, k in enumerate(('count', 'diff', 'largest'))}
    out['de_total'] = Guarded.of(torch.float64, (M,), 0x55, seed=13)
    out['root'], out['size'] = Guarded.of(torch.int32, (M, K), 0x55, seed=14), Guarded.of(torch.int32, (M, K), 0x55, seed=15)
    out['de'] = Guarded.of(torch.float64, (M, K), 0x55, seed=16)
    out['size_hist'] = _framed(torch.int64, np.zeros(nbits + 1, dtype=np.int64) if hist is None else hist, 17)
    if labels:
        out['labels'] = Guarded.of(torch.int32, (M, nbits + pad), 0x55, seed=18)
    rc = L.tn_droplets(g_rows.ptr, M, nbits, rows.shape[1], g_ref.ptr, g_ptr.ptr, g_cols.ptr, g_vals.ptr, len(cols), g_field.ptr if g_field else None, K,
                       out['count'].ptr, out['diff'].ptr, out['largest'].ptr, out['de_total'].ptr, out['root'].ptr, out['size'].ptr, out['de'].ptr,
                       out['size_hist'].ptr, out['labels'].ptr if labels else None, nbits + pad, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, _last_error())
    for g in [g_rows, g_ref, g_ptr, g_cols, g_vals] + ([g_field] if g_field else []) + list(out.values()):
        assert g.intact()
    assert np.array_equal(g_rows.host().view(np.uint64), rows) and np.array_equal(g_ref.host().view(np.uint64), np.asarray(ref, dtype=np.uint64))
    got = {k: g.host() for k, g in out.items()}
    for k in ('count', 'diff', 'largest', 'root', 'size'):
        got[k] = got[k].astype(np.int64)
    if labels:
        assert np.all(got['labels'][:, nbits:] == 0x55555555)
        got['labels'] = np.ascontiguousarray(got['labels'][:, :nbits])
    else:
        got['labels'] = None
    return got


def compare(got, want, exact, rows=slice(None)):
    """The integer outputs exactly; the energies bit for bit (exact) or within the reference's bound."""
    for k in INT_KEYS:
        if got[k] is not None and k != 'size_hist':
            assert np.array_equal(got[k], want[k][rows]), k
    for k in ('de', 'de_total'):
        if exact:
            assert same_bits(got[k], want[k][rows]), k
        else:
            err, bound = np.abs(got[k] - want[k][rows]), want[k + '_bound'][rows]
            print('%s: largest error / bound = %.3g' % (k, float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))))
            assert np.all(err <= bound), k
            assert not np.any(np.signbit(got[k][got[k] == 0]))           # a zero energy is +0.0


# ---------------------------------------------------------------------------------------------- 1. kernel against the reference
@pytest.mark.parametrize('case', dr.CASES, ids=CASE_IDS)
def test_kernel_against_the_reference(case):
    """Every output of the call against the reference; and from the device's own output, for every row: the sizes of all droplets add up
    to the differing bits, the labels reproduce the sizes by bincount and the roots as the first entry of each label, the roots ascend,
    the row that equals the reference has no droplet and only empty slots."""
    c = dr.case_inputs(case)
    n, K = c['nbits'], c['K']
    got, want = droplets_device(**c), dr.case_reference(case)
    compare(got, want, c['exact'])
    assert np.array_equal(got['size_hist'], want['size_hist'])
    assert got['size_hist'][0] == 0 and got['size_hist'].sum() == got['count'].sum()
    assert (got['size_hist'] * np.arange(n + 1)).sum() == got['diff'].sum()
    full = xr.popcounts(c['rows'] ^ np.concatenate([c['ref'], np.zeros(xr.PAD, dtype=np.uint64)])[None, :], n)
    assert np.array_equal(got['diff'], full)
    assert got['count'][0] == 0 and got['diff'][0] == 0 and got['largest'][0] == 0 and got['diff'][1] == n
    assert np.all(got['root'][0] == -1) and np.all(got['size'][0] == 0) and same_bits(got['de'][0], np.zeros(K)) and same_bits(got['de_total'][:1], np.zeros(1))
    for m in range(len(c['rows'])):
        cnt, lab = int(got['count'][m]), got['labels'][m]
        assert lab.max(initial=-1) == cnt - 1
        sizes = np.bincount(lab[lab >= 0], minlength=cnt)
        assert sizes.sum() == got['diff'][m] and sizes.max(initial=0) == got['largest'][m] and np.all(sizes[:cnt] > 0)
        k = min(cnt, K)
        assert np.array_equal(got['size'][m, :k], sizes[:k]) and np.all(got['size'][m, k:] == 0) and np.all(got['root'][m, k:] == -1)
        firsts = np.array([np.flatnonzero(lab == d)[0] for d in range(k)], dtype=np.int64)
        assert np.array_equal(got['root'][m, :k], firsts) and np.all(np.diff(firsts) > 0)
    if case[0] == 'alternating' and n >= 63:
        assert got['count'][2] == (n + 1) // 2 > K and got['count'][3] == n // 2 and np.all(got['size'][2:4] == 1)
    if case[0] == 'path-full':
        assert got['count'][1] == 1 and got['largest'][1] == n
    if case[0] == 'path-gap' and n >= 63:
        assert got['count'][2] == 2 and got['size'][2, :2].tolist() == [n // 2, n - n // 2 - 1]


# ---------------------------------------------------------------------------------------------- 2. slots, fields, labels
@pytest.mark.parametrize('K', [0, 1, 200])
def test_slots(K):
    """No slot, one slot, more slots than any row has droplets: the counts, the totals and size_hist do not depend on K."""
    c = dr.case_inputs(CHIMERA)
    want = dr.run(c['rows'], c['ref'], 128, c['rowptr'], c['cols'], c['vals'], c['field'], K)
    got = droplets_device(**dict(c, K=K))
    compare(got, want, True)
    base = dr.case_reference(CHIMERA)
    assert np.array_equal(got['size_hist'], base['size_hist']) and same_bits(got['de_total'], base['de_total']) and np.array_equal(got['count'], base['count'])
    assert got['root'].shape == (len(c['rows']), K) and (K < 200 or np.all(got['count'] < K))


@pytest.mark.parametrize('n', [130, 4097])
def test_null_field_null_labels_and_a_label_stride(n):
    case = ('cliques', n)
    c = dr.case_inputs(case)
    want = dr.case_reference(case)
    got = droplets_device(**c, labels=False)
    assert got['labels'] is None
    compare(got, want, True)
    got = droplets_device(**c, pad=5)                                    # ldl = nbits + 5: the entries behind a row's labels are left alone
    compare(got, want, True)
    free = dr.run(c['rows'], c['ref'], n, c['rowptr'], c['cols'], c['vals'], None, c['K'])
    got = droplets_device(**dict(c, field=None))
    compare(got, free, True)
    assert not same_bits(free['de_total'], want['de_total'])


def test_size_hist_is_added_to():
    c = dr.case_inputs(CHIMERA)
    start = np.arange(129, dtype=np.int64) * 1000003 + 2 ** 40
    got = droplets_device(**c, hist=start)
    assert np.array_equal(got['size_hist'] - start, dr.case_reference(CHIMERA)['size_hist'])


# ---------------------------------------------------------------------------------------------- 3. slicing
@pytest.mark.parametrize('case', [CHIMERA, ('real', 128), ('real', 4096), ('real', 4097)], ids=['chimera-128', 'real-128', 'real-4096', 'real-4097'])
def test_slicing(case):
    """M cut into calls of different sizes (one row, three rows, the rest; the rows reversed): the same bits in every per-row output,
    real couplings included; the size counts accumulated over the calls equal those of the single call."""
    c = dr.case_inputs(case)
    whole = droplets_device(**c)
    M = len(c['rows'])
    per_row = ('count', 'diff', 'largest', 'de_total', 'root', 'size', 'de', 'labels')
    hist, parts = np.zeros(c['nbits'] + 1, dtype=np.int64), []
    for lo, hi in ((0, 1), (1, 4), (4, M)):
        part = droplets_device(**dict(c, rows=c['rows'][lo:hi]), hist=hist)
        hist = part['size_hist']
        parts.append(part)
    assert np.array_equal(hist, whole['size_hist'])
    for k in per_row:
        assert same_bits(np.concatenate([p[k] for p in parts]), whole[k]), k
    rev = droplets_device(**dict(c, rows=c['rows'][::-1]))
    for k in per_row:
        assert same_bits(rev[k][::-1], whole[k]), k
    assert np.array_equal(rev['size_hist'], whole['size_hist'])


def test_wrapper():
    """ops.droplets on plain device tensors, rows with a stride, the accumulating size counts; its refusals."""
    from tnac4o_amd import ops
    c = dr.case_inputs(CHIMERA)
    want = dr.case_reference(CHIMERA)
    args = [dv(c['ref'].view(np.int64)), dv(c['rowptr']), dv(c['cols']), dv(c['vals']), dv(c['field'])]
    d_rows = dv(c['rows'].view(np.int64))
    got = ops.droplets(d_rows, 128, *args, K=c['K'], labels=True)
    assert got['count'].dtype == torch.int32 and got['de'].dtype == torch.float64 and got['size_hist'].dtype == torch.int64
    host = {k: v.cpu().numpy() for k, v in got.items()}
    compare(host, want, True)
    assert np.array_equal(host['size_hist'], want['size_hist'])
    again = ops.droplets(d_rows[:7], 128, *args[:4], None, 3, got['size_hist'])
    assert again['labels'] is None and again['size_hist'] is got['size_hist'] and again['root'].shape == (7, 3)
    more = dr.run(c['rows'][:7], c['ref'], 128, c['rowptr'], c['cols'], c['vals'], None, 3)
    assert np.array_equal(got['size_hist'].cpu().numpy(), want['size_hist'] + more['size_hist'])
    assert same_bits(again['de'].cpu().numpy(), more['de'])
    none = ops.droplets(d_rows[:0], 128, *args, K=4)
    assert none['count'].numel() == 0 and none['root'].shape == (0, 4) and int(none['size_hist'].sum()) == 0
    with pytest.raises(RuntimeError):
        ops.droplets(d_rows.cpu(), 128, *args)
    with pytest.raises(RuntimeError):
        ops.droplets(d_rows, 128, args[0].cpu(), *args[1:])
    with pytest.raises(TypeError):
        ops.droplets(d_rows, 128, args[0], dv(c['rowptr'][:-1]), *args[2:])
    with pytest.raises(TypeError):
        ops.droplets(d_rows, 128, args[0], args[1], dv(c['cols'].astype(np.int64)), *args[3:])
    with pytest.raises(TypeError):
        ops.droplets(d_rows, 128, args[0], args[1], args[2], dv(c['vals'][:-1]), args[4])
    with pytest.raises(TypeError):
        ops.droplets(d_rows, 128, args[0], args[1], args[2], dv(c['vals'].astype(np.float32)), args[4])
    with pytest.raises(TypeError):
        ops.droplets(d_rows, 128, *args[:4], dv(c['field'][:-1]))
    with pytest.raises(TypeError):
        ops.droplets(d_rows, 128, dv(c['ref'][:1].view(np.int64)), *args[1:])
    with pytest.raises(TypeError):
        ops.droplets(d_rows, 128, *args, size_hist=torch.zeros(128, dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError):
        ops.droplets(d_rows, 64 * d_rows.shape[1] + 1, *args)
    with pytest.raises(ValueError):
        ops.droplets(d_rows, 128, *args, K=-1)


# ---------------------------------------------------------------------------------------------- 4. the public call
def make(name):
    if name.startswith('droplet'):
        return droplet(int(name[-1]), beta=1.0)
    return small(name, 1.0)


ATTRS = (('droplet_count', 'count'), ('droplet_hamming', 'diff'), ('droplet_largest', 'largest'), ('droplet_roots', 'root'), ('droplet_sizes', 'size'))


def check_public(ins, want, K, exact=False):
    """Every stored attribute against public_reference's dict."""
    for attr, key in ATTRS:
        assert np.array_equal(getattr(ins, attr), want[key]), attr
    assert np.array_equal(ins.droplet_size_counts, want['size_hist']) and ins.droplet_size_counts.dtype == np.int64
    assert np.array_equal(ins.droplet_truncated, np.flatnonzero(want['count'] > K))
    for attr, key in (('droplet_energies', 'de'), ('droplet_energy_total', 'de_total')):
        err = np.abs(getattr(ins, attr) - want[key])
        print('%s: largest error %.3g, largest bound %.3g' % (attr, float(err.max(initial=0.0)), float(want[key + '_bound'].max(initial=0.0))))
        assert np.all(err <= want[key + '_bound']), attr
        if exact:
            assert same_bits(getattr(ins, attr), want[key])


@pytest.mark.parametrize('name', ['ising3x3', 'chimera2x2', 'droplet0', 'droplet1'])
def test_public_call(name):
    """After sample_boltzmann(M=64) and after relax_samples(mode='quench'): every attribute against the reference built from J0 alone;
    the total against energy - droplet_reference_energy; labels reproduce the sizes; reference= as an index and as bits agree; states=
    and chunk= give the same; states and energy are unchanged, bit for bit."""
    ins = make(name)
    ins.sample_boltzmann(M=64, Dmax=4, seed=31)
    for step in ('sampled', 'quenched'):
        if step == 'quenched':
            ins.relax_samples(mode='quench')
        states, energy = np.copy(ins.states), np.copy(ins.energy)
        bits = ins.binary_states()
        lowest = int(np.argmin(energy))
        K = 4 if step == 'sampled' else 64
        count = ins.calculate_droplets(max_droplets=K, labels=True)
        want = dr.public_reference(ins, bits, bits[lowest], K)
        assert count is ins.droplet_count and count.shape == (64,)
        check_public(ins, want, K)
        assert same_bits(ins.states, states) and same_bits(ins.energy, energy)
        act = np.flatnonzero(bits[0] != 2)
        assert np.array_equal(ins.droplet_reference[act], bits[lowest][act]) and ins.droplet_reference.shape == (ins.L,)
        assert ins.droplet_count[lowest] == 0 and ins.droplet_hamming[lowest] == 0
        # the droplets add up to the energy difference.  Three computed numbers meet here: sum dE (t_d terms), energy[m] and
        # droplet_reference_energy (each a sum of the model's t_E couplings and fields, in an order of its own).  The bound is the one
        # of the kernel's energies, (t + 1) 2^-52 sum |terms|, over ALL the terms of the comparison: t = t_d + 2 t_E.
        J0 = np.asarray(ins.J0)
        t_E, s_E = np.count_nonzero(np.triu(J0)), float(np.abs(np.triu(J0)).sum())
        bound = (want['nterms'] + 2 * t_E + 1) * dr.EPS * (want['abs_sum'] + 2.0 * s_E)
        err = np.abs(ins.droplet_energy_total - (energy - ins.droplet_reference_energy))
        print('%s %s: |sum dE - (E - E_ref)| largest %.3g, smallest bound %.3g; the sum\'s own bound alone: largest %.3g'
              % (name, step, float(err.max()), float(bound.min()), float(want['de_total_bound'].max())))
        assert np.all(err <= bound)
        # labels
        lab = ins.droplet_labels
        assert lab.shape == (64, ins.L) and lab.dtype == np.int32 and np.array_equal(lab, want['labels'])
        assert np.array_equal(lab >= 0, (bits != bits[lowest][None, :]) & (bits != 2))
        for m in range(64):
            sizes = np.bincount(lab[m][lab[m] >= 0], minlength=int(count[m]))
            k = min(int(count[m]), K)
            assert np.array_equal(sizes[:k], ins.droplet_sizes[m, :k]) and sizes.sum() == ins.droplet_hamming[m] and len(sizes) == count[m]
        kept = {a: np.copy(getattr(ins, a)) for a in ('droplet_count', 'droplet_roots', 'droplet_sizes', 'droplet_energies', 'droplet_energy_total',
                                                      'droplet_size_counts', 'droplet_labels', 'droplet_reference')}
        e_ref = ins.droplet_reference_energy
        for kw in (dict(reference=lowest), dict(reference=bits[lowest]), dict(reference=bits[lowest].astype(np.int64), chunk=7),
                   dict(states=states.astype(np.int64) & 0xff if states.dtype.itemsize == 1 else states, chunk=64)):
            ins.calculate_droplets(max_droplets=K, labels=True, **kw)
            for a, v in kept.items():
                assert same_bits(getattr(ins, a), v), (kw.keys(), a)
            assert ins.droplet_reference_energy == e_ref
        ins.calculate_droplets(reference=5, max_droplets=K)             # another reference, no labels
        assert ins.droplet_labels is None and ins.droplet_count[5] == 0
        check_public(ins, dr.public_reference(ins, bits, bits[5], K), K)
        assert same_bits(ins.states, states) and same_bits(ins.energy, energy)


def test_public_call_on_given_states_with_integer_couplings():
    """C8_J124_001 (512 spins, couplings in +-1, 2, 4: exact): 16 given random states against a given reference, nothing stored before;
    every energy bit for bit, and the total equals the energy difference exactly."""
    import golden_inputs as gi
    import tnac4o_amd
    ins = tnac4o_amd.tnac4o(mode='Ising', Nx=8, Ny=8, Nc=8, J=gi.j124_J(1), beta=1.0)
    rng = np.random.default_rng(8)
    qs = ins._cell_sizes()[ins.order]
    ref_state = rng.integers(0, qs[None, :], size=(1, qs.size))
    given = np.repeat(ref_state, 16, axis=0)
    for m in range(1, 16):                                              # row 0 equals the reference, the others differ in 1 .. 15 cells
        cells = rng.choice(qs.size, m, replace=False)
        given[m, cells] = (given[m, cells] + 1 + rng.integers(0, qs[cells] - 1)) % qs[cells]
    ins.states = np.concatenate([ref_state, given])
    bits = ins.binary_states()
    ins.states = np.zeros((0, qs.size), dtype=np.int64)
    ins.calculate_droplets(reference=bits[0], states=given, max_droplets=32, labels=True)
    want = dr.public_reference(ins, bits[1:], bits[0], 32)
    check_public(ins, want, 32, exact=True)
    assert np.array_equal(ins.droplet_labels, want['labels']) and ins.states.shape == (0, qs.size)
    from tnac4o_amd.droplets_of_states import reference_energy
    E = np.array([reference_energy(ins.J0, b) for b in bits[1:]])
    assert np.array_equal(ins.droplet_energy_total, E - ins.droplet_reference_energy) and ins.droplet_count[0] == 0 and np.all(ins.droplet_count[1:] > 0)
