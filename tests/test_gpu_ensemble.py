"""The ensemble unit on the device: pk_ensemble_moments and pk_ensemble_points bit for bit against their numpy float64 restatement
(tests/ensemble_np.py) at the sizes where the kernels change route: one and four floats per thread, the register form up to
PK_ENS_REG_MEMBERS members and the two-read form above it, a length one group beyond a full pass of the capped grid, 255 / 256 / 257
members around the workgroup of the point kernel, and one point more than its grid."""
import functools

import numpy as np
import pytest
import torch

import ensemble_np as enp

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
REG, CAP, THREADS, POINT_CAP = 32, 4096, 256, 65536              # PK_ENS_REG_MEMBERS, PK_ENS_GRID_CAP, the workgroup, PK_ENS_POINT_GRID_CAP


def G(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV, dtype)          # a copy: the cached inputs are read-only


def same_bits(got, want):
    got = got.cpu().numpy()
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@functools.lru_cache(maxsize=None)
def _stack(S, n):
    g = np.random.default_rng(S * 7919 + n)
    a = (g.standard_normal((S, n)) * g.uniform(0.01, 30.0, (1, n)) + g.standard_normal((1, n))).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _moments(S, n, ddof):
    m, s = enp.moments(_stack(S, n), ddof)
    m.setflags(write=False)
    s.setflags(write=False)
    return m, s


def test_the_constants_here_are_the_headers():
    from infantposeestimation_gaussianbias_amd import _lib
    c = _lib.CONSTANTS
    assert (c["PK_ENS_REG_MEMBERS"], c["PK_ENS_GRID_CAP"], c["PK_ENS_POINT_GRID_CAP"]) == (REG, CAP, POINT_CAP)


# ------------------------------------------------------------------------------------------------ pk_ensemble_moments
# (1, 1) and (2, 3): less than one group; 17 * 16 * 12 = 3 264: the flagship's member count on four floats per thread, register form;
# REG and REG + 1 members: the last size of the register form and the first of the two-read form, at L = 1 021 and 1 025 (one float per
# thread, ragged last workgroup) and at L = 1 024 (four floats per thread)
SHAPES = [(1, 1), (2, 3), (30, 17 * 16 * 12), (REG, 1021), (REG + 1, 1021), (REG, 1025), (REG + 1, 1025), (REG, 1024), (REG + 1, 1024),
          (REG + 5, 17 * 16 * 12)]


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_moments_equal_the_restatement_bitwise(shape, ddof):
    from infantposeestimation_gaussianbias_amd import hipops
    S, n = shape
    if S < 1 + ddof:
        with pytest.raises(RuntimeError, match="at least 2"):
            hipops.ensemble_moments(G(_stack(S, n)), ddof=ddof)
        return
    st = G(_stack(S, n))
    before = st.clone()
    mean, std = hipops.ensemble_moments(st, ddof=ddof)
    want_m, want_s = _moments(S, n, ddof)
    assert mean.dtype == std.dtype == torch.float32 and same_bits(mean, want_m) and same_bits(std, want_s)
    assert torch.equal(st, before)                                # the stack is unchanged
    if n == 17 * 16 * 12:                                         # (S, K, h, w) is the same call
        m4, s4 = hipops.ensemble_moments(st.view(S, 17, 16, 12), ddof=ddof)
        assert tuple(m4.shape) == (17, 16, 12) and torch.equal(m4.reshape(-1), mean) and torch.equal(s4.reshape(-1), std)


@pytest.mark.parametrize("S", [2, REG + 1])
def test_moments_read_views_and_unaligned_stacks(S):
    """A member stride above L on both routes (a multiple of four floats keeps the 16-byte route, L + 3 does not), and a base pointer one
    float off, which takes the one-float route: the same bits as the contiguous stack."""
    from infantposeestimation_gaussianbias_amd import hipops
    n = 1024
    want_m, want_s = _moments(S, n, 0)
    for pad in (8, 3):
        wide = torch.full((S, n + pad), float("nan"), device=DEV)
        wide[:, :n] = G(_stack(S, n))
        view = wide[:, :n]
        assert view.stride(0) == n + pad and not view.is_contiguous()
        mean, std = hipops.ensemble_moments(view)
        assert same_bits(mean, want_m) and same_bits(std, want_s), pad
        assert bool(torch.isnan(wide[:, n:]).all())
    flat = torch.empty(S * n + 1, device=DEV)
    off = flat[1:].view(S, n)
    off.copy_(G(_stack(S, n)))
    assert off.data_ptr() % 16 == 4
    mean, std = hipops.ensemble_moments(off)
    assert same_bits(mean, want_m) and same_bits(std, want_s)
    out = (torch.empty(n, device=DEV), torch.empty(n, device=DEV))          # into given outputs
    back = hipops.ensemble_moments(off, out=out)
    assert back[0].data_ptr() == out[0].data_ptr() and same_bits(out[0], want_m) and same_bits(out[1], want_s)
    with pytest.raises(RuntimeError, match="overlaps the stack"):
        hipops.ensemble_moments(off, out=(off[0], out[1]))


@pytest.mark.parametrize("n", [CAP * THREADS * 4 + 4, CAP * THREADS + 1])
def test_moments_stride_over_more_than_one_pass_of_the_capped_grid(n):
    """4 096 workgroups of 256 threads at most: one 16-byte group (four floats per thread), or one float (n odd: one per thread), more
    than a full pass covers, with S = 2."""
    from infantposeestimation_gaussianbias_amd import hipops
    st = np.random.default_rng(n).standard_normal((2, n)).astype(np.float32)
    mean, std = hipops.ensemble_moments(G(st), ddof=1)
    want_m, want_s = enp.moments(st, 1)
    assert same_bits(mean, want_m) and same_bits(std, want_s)
    assert bool(std[-1] != 0) and bool(std[CAP * THREADS * (4 if n % 4 == 0 else 1) - 1] != 0)


@pytest.mark.parametrize("S", [5, REG + 1])
def test_moments_propagate_nan_and_inf(S):
    from infantposeestimation_gaussianbias_amd import hipops
    st = np.array(_stack(S, 1024))
    st[2, 10], st[S - 1, 700], st[0, 701], st[1, 701] = np.nan, np.inf, np.inf, -np.inf
    mean, std = hipops.ensemble_moments(G(st))
    want_m, want_s = enp.moments(st)
    mean, std = mean.cpu().numpy(), std.cpu().numpy()
    for got, want in ((mean, want_m), (std, want_s)):             # a NaN has no canonical sign or payload: the same places, and the
        nan = np.isnan(want)                                      # same bits everywhere else
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))
    assert np.flatnonzero(np.isnan(mean)).tolist() == [10, 701]   # a NaN member; +inf and -inf
    assert np.flatnonzero(np.isnan(std)).tolist() == [10, 700, 701] and mean[700] == np.inf


# ------------------------------------------------------------------------------------------------ pk_ensemble_points
MIN_CONF = 0.2


@functools.lru_cache(maxsize=None)
def _members(S, M):
    """Positions on a quarter-pixel grid around per-point centres (so that some land exactly on the radius 1.25), peaks in [0, 1).
    Point 0: every seventh member has a NaN coordinate, every fifth a peak exactly at MIN_CONF (valid), and for S > 2 every fourth from
    the second an infinite peak (invalid).  For M > 1: point M - 1 has peaks below MIN_CONF only, point M - 2 identical members."""
    g = np.random.default_rng(S * 131 + M)
    centre = g.integers(2, 40, (M, 2)).astype(np.float64)
    c = (centre[None] + g.integers(-8, 9, (S, M, 2)) * 0.25).astype(np.float32)
    cf = g.uniform(0.0, 1.0, (S, M)).astype(np.float32)
    c[::7, 0, g.integers(0, 2)] = np.nan
    cf[::5, 0] = np.float32(MIN_CONF)                             # exactly min_conf: valid
    if S > 2:
        cf[1::4, 0] = np.inf                                      # a conf that is not finite: invalid
    if M > 1:
        cf[:, M - 1] = g.uniform(0.0, 0.19, S)
        c[:, M - 2, :] = c[0, M - 2, :]                           # all members identical
        cf[:, M - 2] = cf[0, M - 2] = 0.5
    for a in (centre, c, cf):
        a.setflags(write=False)
    return c, cf, centre


@pytest.mark.parametrize("with_centre", [True, False])
@pytest.mark.parametrize("with_conf", [True, False])
@pytest.mark.parametrize("M", [1, 17])
@pytest.mark.parametrize("S", [1, 2, 30, 255, 256, 257, 1000])
def test_points_equal_the_restatement_bitwise(S, M, with_conf, with_centre):
    from infantposeestimation_gaussianbias_amd import hipops
    c, cf, centre = _members(S, M)
    for ddof in (0, 1):
        got = hipops.ensemble_points(G(c), G(cf) if with_conf else None, G(centre, F64) if with_centre else None, MIN_CONF, 1.25, ddof)
        want = enp.points(c, cf if with_conf else None, centre if with_centre else None, MIN_CONF, 1.25, ddof)
        assert tuple(got.shape) == (M, 12) and got.dtype == F64
        got = got.cpu().numpy()
        assert np.array_equal(got, want), (ddof, np.argwhere(got != want)[:5])
        ok = np.isfinite(c[:, 0]).all(1)                          # point 0: NaN coordinates, and with conf an inf and values at min_conf
        if with_conf:
            ok = ok & np.isfinite(cf[:, 0]) & (cf[:, 0] >= np.float32(MIN_CONF))
        if ok.sum() >= 1 + ddof:
            assert got[0, 0] == ok.sum() < S
        else:
            assert not got[0].any()
        if not with_conf:
            assert not got[:, 8:11].any()
        if M > 1:
            if with_conf:
                assert not got[M - 1].any()                       # no member is valid: a row of zeros
            if S >= 1 + ddof:                                     # identical members: no spread at all, everybody agrees with the mean
                row = got[M - 2]
                assert row[0] == S and row[3:8].tolist() == [0.0] * 5 and row[9] == 0.0
                assert (row[11] == S) or with_centre


def test_points_count_a_member_exactly_at_the_radius_and_stride_over_more_points_than_the_grid():
    from infantposeestimation_gaussianbias_amd import hipops
    c = np.array([[[3.0, 4.0]], [[0.0, 0.0]], [[3.0, 4.25]], [[-5.0, 0.0]]], np.float32)
    centre = np.zeros((1, 2))
    got = hipops.ensemble_points(G(c), None, G(centre, F64), 0.0, 5.0).cpu().numpy()
    assert np.array_equal(got, enp.points(c, None, centre, 0.0, 5.0)) and got[0, 0] == 4 and got[0, 11] == 3      # 25 <= 25 counts
    assert hipops.ensemble_points(G(c), None, G(centre, F64), 0.0, 0.0).cpu().numpy()[0, 11] == 1                # radius 0: the centre itself
    # 65 536 workgroups at most: with one point more the first workgroup takes a second point.  S = 2: threads 0 and 1 hold one member
    # each and the butterfly's last step adds them
    M = POINT_CAP + 1
    g = np.random.default_rng(4)
    c = g.standard_normal((2, M, 2)).astype(np.float32)
    cf = g.uniform(0, 1, (2, M)).astype(np.float32)
    got = hipops.ensemble_points(G(c), G(cf), None, 0.0, 1.0, 1).cpu().numpy()
    rows = np.r_[0:64, POINT_CAP - 2:M]
    assert np.array_equal(got[rows], enp.points(c[:, rows], cf[:, rows], None, 0.0, 1.0, 1))
    x = c.astype(np.float64)
    mean = (x[0] + x[1]) / 2.0
    d0, d1 = x[0] - mean, x[1] - mean
    assert np.array_equal(got[:, 0], np.full(M, 2.0)) and np.array_equal(got[:, 1:3], mean)
    assert np.array_equal(got[:, 3:5], d0 * d0 + d1 * d1) and np.array_equal(got[:, 5], d0[:, 0] * d0[:, 1] + d1[:, 0] * d1[:, 1])
    assert np.array_equal(got[:, 10], np.minimum(cf[0], cf[1]).astype(np.float64))


def test_op_layer_checks_shapes_and_writes_into_out():
    from infantposeestimation_gaussianbias_amd import hipops
    from infantposeestimation_gaussianbias_amd._lib import PoseKernelError
    c, cf, centre = _members(30, 17)
    table = torch.full((19, 12), -1.0, dtype=F64, device=DEV)
    back = hipops.ensemble_points(G(c), G(cf), G(centre, F64), MIN_CONF, 1.25, out=table[1:18])
    assert back.data_ptr() == table[1:18].data_ptr() and bool((table[0] == -1).all()) and bool((table[18] == -1).all())
    assert np.array_equal(table[1:18].cpu().numpy(), enp.points(c, cf, centre, MIN_CONF, 1.25))
    with pytest.raises(PoseKernelError, match=r"\(S, M, 2\)"):
        hipops.ensemble_points(G(c)[..., :1])
    with pytest.raises(PoseKernelError, match="conf"):
        hipops.ensemble_points(G(c), G(cf)[:, :3])
    with pytest.raises(PoseKernelError, match="centre"):
        hipops.ensemble_points(G(c), None, G(centre))             # float32
    with pytest.raises(PoseKernelError, match="radius"):
        hipops.ensemble_points(G(c), radius=-1.0)
    with pytest.raises(PoseKernelError, match="expected"):
        hipops.ensemble_moments(G(c).double())
    empty_m, empty_s = hipops.ensemble_moments(torch.empty(3, 0, 4, device=DEV))
    assert tuple(empty_m.shape) == tuple(empty_s.shape) == (0, 4)
    assert tuple(hipops.ensemble_points(torch.empty(3, 0, 2, device=DEV)).shape) == (0, 12)
