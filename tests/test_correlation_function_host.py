"""Host side of tnac4o.calculate_correlation_function: the model-frame mapping of the line tables under the four rotations, the
planning of the stack groups and the argument checks.  No GPU here."""
import functools

import numpy as np
import pytest

import correlation_function_ref as cfr
import marginals_ref as mr


def _make(case):
    import tnac4o_amd
    from tnac4o_amd import auxx
    if case == 'ising3x3':
        J = mr.ising_3x3_nc2()
        return tnac4o_amd.tnac4o(mode='Ising', Nx=3, Ny=3, Nc=2, J=J, beta=0.7), J
    J = auxx.synthetic_rmf(3, 2, 3, 23)                 # 3 columns, 2 rows: rows and columns differ in length
    return tnac4o_amd.tnac4o(mode='RMF', Nx=3, Ny=2, J=J, beta=0.7), J


@functools.lru_cache(maxsize=1)
def _exact_ising3x3():
    return cfr.exact_line_ising(mr.ising_3x3_nc2(), 3, 3, 2, 0.7)


@pytest.mark.parametrize('rot', [0, 1, 2, 3])
def test_model_frame_mapping_ising(rot):
    from tnac4o_amd.tnac4o import model_line_correlations
    ins, J = _make('ising3x3')
    pairs, dist, C, _ = _exact_ising3x3()
    assert pairs.shape[0] == 64 and set(dist) == {1, 2}          # 18 pairs of cells; spin 9 is inactive: 14 * 4 + 4 * 2
    ins.rotate_graph(rot)
    got = [model_line_correlations(cfr.enum_line_tables(ins, lines), ins.order, ins.Nx, ind=ins.ind, Nc=ins.Nc)
           for lines in ('rows', 'columns')]
    gp = np.concatenate([g[0] for g in got])
    idx = np.lexsort((gp[:, 1], gp[:, 0]))
    assert gp.dtype == np.int64 and np.array_equal(gp[idx], pairs)
    assert np.array_equal(np.concatenate([g[1] for g in got])[idx], dist)
    assert float(np.max(np.abs(np.concatenate([g[2] for g in got])[idx] - C))) <= 1e-13
    for g in got:                                                 # each part comes back sorted
        assert np.array_equal(g[0], g[0][np.lexsort((g[0][:, 1], g[0][:, 0]))])


@pytest.mark.parametrize('rot', [0, 1, 2, 3])
def test_model_frame_mapping_rmf(rot):
    from tnac4o_amd.tnac4o import model_line_correlations
    ins, J = _make('rmf3x2')
    exact = cfr.exact_line_rmf(J, 0.7)
    assert len(exact) == 9
    ins.rotate_graph(rot)
    got = {}
    for lines in ('rows', 'columns'):
        part = model_line_correlations(cfr.enum_line_tables(ins, lines), ins.order, ins.Nx, Nx_model=ins.Nx_model)
        assert not set(part) & set(got)
        got.update(part)
    assert sorted(got) == sorted(exact)
    for key, P in exact.items():
        assert got[key].shape == P.shape and float(np.max(np.abs(got[key] - P))) <= 1e-13, key


def test_mapping_rejects_cells_off_a_line():
    from tnac4o_amd.tnac4o import model_line_correlations
    with pytest.raises(ValueError):
        model_line_correlations({(0, 4): np.ones((3, 3)) / 9}, np.arange(6), 3, Nx_model=3)
    with pytest.raises(ValueError):
        model_line_correlations({(2, 2): np.ones((3, 3)) / 9}, np.arange(6), 3, Nx_model=3)


def test_group_planning():
    from tnac4o_amd.tnac4o import _plan_line_groups
    assert _plan_line_groups([], 1, 1) == [(0, 0)]
    assert _plan_line_groups([8] * 15, 15, 121) == [(0, 15)]
    assert _plan_line_groups([8] * 15, 15, 120) == [(0, 14), (14, 15)]
    assert _plan_line_groups([8] * 3, 3, 9) == [(0, 1), (1, 2), (2, 3)]
    assert _plan_line_groups([8] * 15, 1, 17) == [(0, 15)]        # reach 1: two neighbouring start cells at a time
    assert _plan_line_groups([2, 0, 5, 1], 4, 7) == [(0, 2), (2, 4)]
    with pytest.raises(MemoryError):
        _plan_line_groups([8] * 3, 3, 8)


@pytest.mark.parametrize('case', ['ising3x3', 'rmf3x2'])
def test_argument_validation(case):
    ins, _ = _make(case)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError):
            ins.calculate_correlation_function(max_distance=bad)
    for bad in ('diagonals', 'row', None):
        with pytest.raises(ValueError):
            ins.calculate_correlation_function(lines=bad)
    assert ins.rotation == 0 and np.array_equal(ins.order, np.arange(ins.Nx * ins.Ny))
