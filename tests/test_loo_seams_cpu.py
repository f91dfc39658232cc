"""CPU companion of tests/test_loo_seams_gpu.py: what that file's cases rest on, checked without a device.  The shapes
it names give the S, M, splits, padded lengths, band groups and select launches it says they give, by the host build of
csrc/mbb_psis.hip.h (tests/_loo_host.cpp) and by pw_run's rules restated; and its one-band inputs, with the oracle's
band fluxes in place of the device's, take the smoothed path in the reference alone and keep the float64 restatement
within 1e-9 / 64 of the longdouble one -- the condition the GPU file asserts of its bound, met before any device is
involved."""
import numpy as np
import pytest

import _loo_ref as LR
from _loo_cases import (SEAM_DELTA1, VARIANTS, _chain, _columns, _data, _groups, _oracle_ll_and_z, _seam_nan_rows,
                        _selects)
from test_loo_cpu import Host

NAME, OPTHIN, NOALPHA = VARIANTS[1]
# every (S, M) of the GPU file: its one-band windows, the four-band ones, the [2, 64, 180] window, the 256 sources
NAMED = ((16384, 384), (16385, 385), (90000, 900), (29400, 515), (116508, 1024), (116509, 1025), (1864135, 4096),
         (1863135, 4095), (1408, 113), (25, 5), (16400, 385))


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    try:
        return Host(tmp_path_factory.mktemp("loo_seams_host"))
    except RuntimeError as e:
        pytest.skip(str(e))


def test_tail_and_grid_lengths_at_the_named_sizes(H):
    """_loo_ref.tail_len and the host build's ps_tail_len agree on M at every S the GPU file names and at S - 1 and
    S + 1, the named M included; ps_grid_len is 62 at M = 1024 and 94 = kGridMax at M = 4096 = kTailMax."""
    for S, M in NAMED:
        assert H.lib.ps_host_tail_len(S) == M == LR.tail_len(S), (S, M)
        for near in (S - 1, S + 1):
            assert H.lib.ps_host_tail_len(near) == LR.tail_len(near), near
    # the seams themselves: M = 384 is the last tail of P = 512 the first split holds alone, 1024 -> 1025 crosses P
    assert LR.tail_len(116507) == 1024 and LR.tail_len(116509) == 1025 and LR.tail_len(1864136) == 4097
    assert H.lib.ps_host_grid_len(1024) == 62 and H.lib.ps_host_grid_len(4096) == 94 == H.grid_max and H.tail_max == 4096


def test_shapes_give_the_splits_windows_and_groups_they_are_named_for():
    """pw_run's rules restated on the GPU file's shapes: splits = min(64, ceil(n / 16384)) below 256 sources and
    per_split = ceil(n / splits); the padded tail length; the windows; the band groups of the [2, 64, 180] chain at
    budgets of 1, 2 and 3 MB and the select launches within them."""
    from mbb_emcee_amd import _native
    for label, (shape, seed, nan, S, M, splits, P) in SEAM_DELTA1.items():
        n = shape[1] * shape[2]
        assert n - nan == S and LR.tail_len(S) == M and min(64, (n + 16383) // 16384) == splits, label
        assert P == 1 << (M - 1).bit_length() and P <= _native.PW_TAIL_MAX, label
        assert np.unique(_seam_nan_rows(shape, nan)).size == nan
    assert SEAM_DELTA1["S max"][0][1] * SEAM_DELTA1["S max"][0][2] == _native.PW_MAX_WINDOW
    assert -(-16385 // 2) == 8193 and min(64, (90000 + 16383) // 16384) == 6 and min(64, (16400 + 16383) // 16384) == 2
    assert 300 * len(range(7, 300, 3)) == 29400 and 64 * len(range(4, 180, 8)) == 1408
    cells = 2 * 64 * 180
    assert [_groups(12, cells, mb) for mb in (1, 2, 3, 16384)] == [[2] * 6, [5, 5, 2], [8, 4], [12]]
    assert [_groups(8, cells, mb) for mb in (1, 16384)] == [[2] * 4, [8]] and _groups(12, cells, 0) == [1] * 12
    assert [_selects(g) for g in (2, 5, 8, 4, 12)] == [[2], [3, 2], [3, 3, 2], [3, 1], [3, 3, 3, 3]]
    # (a [2, 64, 200] chain gives 2 and 5 as well, but 7 and 5 at 3 MB: no group of four, the plain 3 + 1 select)
    assert [_groups(12, 2 * 64 * 200, mb) for mb in (1, 2, 3)] == [[2] * 6, [5, 5, 2], [7, 5]]


@pytest.mark.parametrize("label", list(SEAM_DELTA1))
def test_one_band_inputs_take_the_smoothed_path(oracle, g_lnl, g_pb, g_res, label):
    """The GPU file's one-band windows on the oracle's band fluxes: S and M as named, k-hat finite (no TAIL_FLAT or
    TAIL_SHORT) in the longdouble and the float64 restatement alike, the same status and tail in both, and their
    distance below 1e-9 / 64.  The 1 864 135-entry windows are included: the oracle makes their ll in a few seconds."""
    shape, seed, nan, S, M, splits, P = SEAM_DELTA1[label]
    data = _data(oracle, g_lnl, g_pb, g_res[NAME + "/chain"], OPTHIN, NOALPHA, "delta1", 1.0)
    rows = _chain(g_res, NAME, shape, seed=seed)[0].reshape(-1, 5)
    rows[_seam_nan_rows(shape, nan), 0] = np.nan
    ll, z = _oracle_ll_and_z(oracle, data, rows, OPTHIN, NOALPHA)
    ref, f64 = _columns(ll, z)
    r, f = ref[0], f64[0]
    assert r["n_used"] == S == f["n_used"] and r["tail_len"] == M == f["tail_len"]
    assert r["status"] == f["status"] and (r["status"] & (LR.TAIL_FLAT | LR.TAIL_SHORT)) == 0
    assert bool(r["status"] & LR.HAS_NAN) == (nan > 0)
    assert np.isfinite(float(r["khat"])) and np.isfinite(f["khat"]) and np.array_equal(r["tail"], f["tail"])
    spread = LR.distance(f, r)
    print("    %s: k-hat %.4g, float64 restatement vs longdouble %.3g" % (label, float(r["khat"]), spread))
    assert 0.0 < spread < 1e-9 / 64.0
